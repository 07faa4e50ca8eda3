// Host runtime of the decoder: weight repacking/folding, workspace, hipGraph-captured step loop.
//
// One decoder step = 6 launches on the library's own stream:
//   prenet L2 (sgemm relu) -> attention LSTM (sgemm + LSTM epilogue) -> query (sgemm)
//   -> attention (1 WG / sentence) -> decoder LSTM (sgemm + LSTM epilogue)
//   -> fused [mel projection | next step's prenet L1 | stopnet + stop rule] (sgemm).
// Prenet L1 and the stopnet are folded into the mel projection at load time (W1 W_mel and
// w_stop W_mel, fp64), so the reference's mel -> prenet -> ... chain loses two dependent launches.
// Ping-pong activation buffers are bound statically per step parity: three graphs are captured
// per (B, Lmax, max_steps) — one even step, one odd step, and a CHUNK-step run starting even.
// The step index and active count live in device memory in two parity slots {step, n_active}:
// a step reads its own slot and the stop rule writes the other, so no launch ever races on it.
// The host synchronises only at chunk boundaries: the first chunk is the reference's lower
// bound on the step count (min(2L+22, max_steps) per sentence, layers/tacotron2.py:268-277).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "decoder.h"
#include "host_util.h"
#include "resident.h"
#include "sgemm.h"

using namespace tts;

namespace {
constexpr int CHUNK = 8;  // decoder steps per chunk graph
}  // namespace

struct tts_decoder {
    tts_decoder_config cfg{};
    int nmel = 80;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    hipEvent_t ev_sync = nullptr;  // spin_sync (runtime.hip)
    DeviceAllocs dev;
    // packed GEMM weights + logical biases
    float *b_pre1 = nullptr, *b_pre2 = nullptr;  // prenet_type "bn": the folded shifts (else null)
    float *W_pre1 = nullptr, *W_pre2 = nullptr, *W_att = nullptr, *b_att = nullptr, *W_q = nullptr;
    float *W_dec = nullptr, *b_dec = nullptr, *W_melf = nullptr, *b_melf = nullptr;
    // reference-layout small weights
    float *v = nullptr, *v_b = nullptr, *ta_w = nullptr, *ta_b = nullptr, *loc_conv = nullptr, *loc_dense = nullptr;
    float *W_in = nullptr, *att_init = nullptr, *dec_init = nullptr, *go = nullptr;
    // workspace
    int Lcap = 0, Bcap = 0, hist_cap = 0;
    float *enc = nullptr, *Pt = nullptr, *h_att = nullptr, *c_att = nullptr, *h_dec = nullptr, *c_dec = nullptr;
    float *xa = nullptr, *mem = nullptr, *pre1 = nullptr, *q = nullptr, *epart = nullptr;
    // fragment-order mirrors (common.h: frag_idx, ntf m-tiles) of the GEMM inputs for batches
    // above 16: written beside the row-major buffers by their producers, read by the 4-wave
    // batched GEMM (sgemm.h: Seg::pf).  Null when max_batch <= 16.
    int ntf = 0;
    float *xaf = nullptr, *hattf = nullptr, *hdecf = nullptr, *pre1f = nullptr;
    int res_gen = 0;              // resident decoder form: 0 = synthesis configuration, else GEN_* bits
    float* loc_conv_p = nullptr;  // location_conv packed for the general resident form
    bool fast_attention = false;  // attention_uses_epart(): the synthesis configuration's attention
                                  // launch (attention_fm_kernel) and the resident decoder
    float* locf = nullptr;        // location_attn: [Bcap][NLOC][Lcap] location features of the next step
    // resident (persistent, one launch per sentence) batch-1 decoder, resident.h
    bool resident = false;
    ResWeights rw{};
    unsigned long long* gran = nullptr;  // [2][GR_TOTAL] granules, then int status[4]
    long long res_ticks = 0;
    unsigned res_salt = 0;
    float *alpha = nullptr, *att_w = nullptr, *att_cum = nullptr, *u = nullptr, *tail = nullptr;
    int *lens = nullptr, *win_idx = nullptr, *nidx = nullptr, *flag1 = nullptr, *count = nullptr, *done = nullptr;
    int *n_steps = nullptr, *state = nullptr;  // state: [2][2] = {step, n_active} per parity
    float *mel_hist = nullptr, *stop_hist = nullptr, *align_hist = nullptr;
    int* host_flags = nullptr;  // pinned coherent: [0, 3) flags, [3] read-back sequence, [4, 4 + 64) step counts
    int rb_seq = 0;             // the resident run's read-back sequence number (host_flags[3])
    // tts_synth_run: work enqueued behind a resident launch before the host waits for it (the
    // postnet, reading the device step counts); hook_ran reports that it was enqueued
    void (*post_hook)(void*, hipStream_t) = nullptr;
    void* post_ctx = nullptr;
    bool hook_ran = false;
    // tts_synth_run (decoder_set_pipeline_io): device length array, one extra status word to read
    // back, the speculative Griffin-Lim frame-count clamp target
    const int* io_lens = nullptr;
    const int* io_rb_src = nullptr;
    int* io_rb_dst = nullptr;
    int* io_clamp = nullptr;
    int io_clamp_max = 0;
    // relu(W_pre1 go): the step-0 prenet layer 1 of a fresh batch-1 resident run, copied by
    // decoder_init instead of a GEMM launch per sentence (computed by the first such run)
    float* pre1_go = nullptr;
    bool pre1_go_ok = false;
    const float* last_enc_direct = nullptr;  // the last direct run's encoder output (profiling re-runs)
    int last_len_direct = 0;                 // ... and its length (the device copy it read may be reused)
    std::vector<long long> res_trace;        // the last tts_decoder_resident_phases run's event trace
    std::map<std::tuple<int, int, int>, StepGraphs> graphs;
    float last_ms = 0.f;
    bool pipeline = false;  // tts_synth_run: work on the caller's stream
    // tts_synth_run: leave mel / stop / alignments in the histories (decoder_histories) instead of
    // copying them out (the postnet reads the mel history in place)
    bool keep_hist = false;
    int last_steps = 0;
    int last_B = 0, last_Lmax = 0, last_max_steps = 0, last_first = 0;
    int last_steps_done = 0;  // steps of the last batch-1 run (continuous mode), 0 otherwise
    int last_resident = 0;    // the last run used the resident decoder
    int res_timeouts = 0;     // resident runs that timed out a hand-off and re-ran multi-launch
    int res_place_fails = 0;  // consecutive resident runs that stopped on a placement failure
    // resident decoder for batches of 2..RB_MAXB sentences per launch (resident_batch.hip)
    bool rbatch = false;
    int rb_gen = 0;
    float4 *rb_wa = nullptr, *rb_wd = nullptr;
    float* rb_loc = nullptr;                // location weights in the batch kernel's packing (general form)
    long long* rb_prof = nullptr;           // TTS_RB_PROF=1 phase clocks
    unsigned long long* rb_gran = nullptr;  // resident_batch_granules() slots, then int status[4]
    unsigned rb_salt = 0;
    int rb_place_fails = 0;
    ResArgs last_ra{};
    InitArgs last_init{};
};

namespace {

// the largest batch the resident batch decoder takes (consecutive launches of <= RB_MAXB): two
// launches of 4 (2 x 16.6 us per step, round 6) beat the multi-launch step (~44 us at any batch up
// to 64); three do not.  TTS_RB_MAX overrides.
int rb_max_batch() {
    // (set and empty counts as unset; a negative value clamps to 0: no batched resident runs)
    static const int v =
        env_is("TTS_RB_MAX", '\0') ? 2 * RB_MAXB : std::max(0, env_int("TTS_RB_MAX", 2 * RB_MAXB));
    return v;
}

// The batched GEMMs read fragment mirrors above 16 sentences (TTS_FRAG=0: row-major always).
bool frag_on(const tts_decoder* d, int B) {
    static const bool off = env_is("TTS_FRAG", '0');
    return d->xaf && B > 16 && !off;
}

// Mirrors of the state a run starts from (after launch_decoder_init): both parities of xa, h_att
// and h_dec (pre1 is mirrored by the prenet launch that writes it).
tts_status enqueue_frag_sync(tts_decoder* d, int B, hipStream_t s) {
    const int64_t hps = (int64_t)d->Bcap * HATT, xps = (int64_t)d->Bcap * XA;
    const int64_t fh = (int64_t)d->ntf * 16 * HATT, fx = (int64_t)d->ntf * 16 * XA;
    for (int p = 0; p < 2; ++p) {
        struct { const float* src; int64_t ld; int K; float* dst; } jobs[3] = {
            {d->xa + p * xps, XA, XA, d->xaf + p * fx},
            {d->h_att + p * hps, HATT, HATT, d->hattf + p * fh},
            {d->h_dec + p * hps, HDEC, HDEC, d->hdecf + p * fh}};
        for (auto& j : jobs) TTS_HIP(frag_mirror(j.src, j.ld, B, j.K, j.dst, d->ntf, s));
    }
    return TTS_OK;
}

// Launches of one decoder step of parity p (0: even step, 1: odd step).  `ev` (optional, 7
// events) brackets every launch for tts_decoder_profile.
tts_status enqueue_step(tts_decoder* d, int B, int Lmax, int max_steps, int p, hipStream_t s,
                        hipEvent_t* ev = nullptr, int rule = 0) {
    int mark = 0;
#define MARK() \
    if (ev) TTS_HIP(hipEventRecord(ev[mark++], s));
    const int nmel = d->nmel;
    const int q = 1 - p;
    const int64_t hps = (int64_t)d->Bcap * HATT;  // ping-pong slot strides
    const int64_t xps = (int64_t)d->Bcap * XA;
    float* h_att_cur = d->h_att + p * hps;
    float* h_att_prev = d->h_att + q * hps;
    float* h_dec_cur = d->h_dec + p * hps;
    float* h_dec_prev = d->h_dec + q * hps;
    float* xa_cur = d->xa + p * xps;   // [prenet_t | ctx_{t-1}]
    float* ctx_cur = d->xa + q * xps + PRE;  // ctx_t (row stride XA)
    int* st_cur = d->state + 2 * p;
    // fragment mirrors of the same buffers (batches above 16)
    const bool fr = frag_on(d, B);
    const int64_t fh = (int64_t)d->ntf * 16 * HATT, fx = (int64_t)d->ntf * 16 * XA;
    const int64_t fchunk = (int64_t)d->ntf * 256;  // floats per 16-column chunk of a mirror
    float* hattf_cur = fr ? d->hattf + p * fh : nullptr;
    float* hattf_prev = fr ? d->hattf + q * fh : nullptr;
    float* hdecf_cur = fr ? d->hdecf + p * fh : nullptr;
    float* hdecf_prev = fr ? d->hdecf + q * fh : nullptr;
    float* xaf_cur = fr ? d->xaf + p * fx : nullptr;
    float* ctxf_cur = fr ? d->xaf + q * fx + (PRE / 16) * fchunk : nullptr;  // ctx_t: xa columns PRE..
    SGemmArgs g{};
    g.B = B;
    g.step = st_cur;
    g.done = d->done;
    g.out_par = -1;
    g.ntf = d->ntf;
    // 1) prenet layer 2 -> xa_cur[b][0:256]   (common_layers.py:77-83; dropout off in eval)
    {
        SGemmArgs a = g;
        a.seg[0] = Seg{d->pre1, PRE, PRE, fr ? d->pre1f : nullptr};
        a.nseg = 1;
        a.W = d->W_pre2; a.K = PRE; a.N = PRE; a.act = ACT_RELU; a.bias = d->b_pre2;
        a.out = xa_cur; a.ldo = XA;
        a.outf = xaf_cur; a.outf_k0 = 0;
        MARK();
        TTS_HIP(sgemm_launch(a, ROLE_PRENET, s));
    }
    // 2) attention LSTM: x = [prenet_t | ctx_{t-1}], h = h_att_{t-1}   (tacotron2.py:195-197)
    {
        SGemmArgs a = g;
        a.seg[0] = Seg{xa_cur, XA, XA, xaf_cur};
        a.seg[1] = Seg{h_att_prev, HATT, HATT, hattf_prev};
        a.nseg = 2;
        a.W = d->W_att; a.K = XA + HATT; a.N = 4 * HATT; a.bias = d->b_att;
        a.out = h_att_cur; a.ldo = HATT;
        a.outf = hattf_cur; a.outf_k0 = 0;
        a.cell = d->c_att; a.ldc = HATT;
        MARK();
        TTS_HIP(sgemm_launch(a, ROLE_ATT_LSTM, s));
    }
    // 3) processed query = query_layer(h_att_t) (common_layers.py:170/179) and, for the fast
    //    attention path, the energy partials v . tanh(q + P_j) over 16 dims per workgroup
    {
        QEArgs a{};
        a.Wq = d->W_q; a.h = h_att_cur; a.v = d->v; a.Pt = d->Pt; a.lens = d->lens; a.Lcap = d->Lcap;
        // every configuration: the energies as QE_TILES partials per position (with the location
        // term from the previous attention launch's features)
        a.energies = 1;
        a.locf = d->locf; a.loc_dense = d->loc_dense;
        a.q = d->q; a.epart = d->epart; a.step = st_cur;
        MARK();
        TTS_HIP(launch_query_energy(a, B, s));
    }
    // 4) attention (energies, norm, forward attention, context -> ctx_t)
    {
        AttnArgs a{};
        const tts_decoder_config& c = d->cfg;
        a.attn_norm = c.attn_norm; a.forward_attn = c.forward_attn; a.trans_agent = c.trans_agent;
        a.forward_attn_mask = c.forward_attn_mask; a.location_attn = c.location_attn; a.windowing = c.windowing;
        a.Lcap = d->Lcap; a.B = B; a.enc_dim = ENC; a.ctx_ld = XA; a.tail_rule = 0;
        a.v = d->v; a.v_b = d->v_b; a.ta_w = d->ta_w; a.ta_b = d->ta_b;
        a.loc_conv = d->loc_conv; a.loc_dense = d->loc_dense;
        a.q = d->q; a.Pt = d->Pt; a.enc = d->enc; a.lens = d->lens;
        a.h_att = h_att_cur;
        a.epart = d->epart; a.locf = d->locf;
        a.sstride = (int64_t)d->Bcap * d->Lcap; a.istride = d->Bcap;
        a.ctx_prev = xa_cur + PRE; a.h_att_prev = h_att_prev;
        a.alpha = d->alpha; a.att_w = d->att_w; a.att_cum = d->att_cum; a.u = d->u; a.win_idx = d->win_idx;
        a.nidx = d->nidx; a.tail = d->tail;
        a.ctx = ctx_cur;  // kernel writes ctx[b*XA + d]
        a.ctxf = fr ? d->xaf + q * fx : nullptr; a.ctxf_k0 = PRE; a.ntf = d->ntf;
        a.align_hist = d->align_hist; a.align_ldb = (int64_t)d->hist_cap * Lmax; a.Lalign = Lmax;
        a.hist_cap = d->hist_cap;
        a.step = st_cur; a.done = d->done;
        MARK();
        TTS_HIP(launch_attention(a, s));
    }
    // 5) decoder LSTM: x = [h_att_t | ctx_t], h = h_dec_{t-1}   (tacotron2.py:206-208)
    {
        SGemmArgs a = g;
        a.seg[0] = Seg{h_att_cur, HATT, HATT, hattf_cur};
        a.seg[1] = Seg{ctx_cur, XA, ENC, ctxf_cur};
        a.seg[2] = Seg{h_dec_prev, HDEC, HDEC, hdecf_prev};
        a.nseg = 3;
        a.W = d->W_dec; a.K = HATT + ENC + HDEC; a.N = 4 * HDEC; a.bias = d->b_dec;
        a.out = h_dec_cur; a.ldo = HDEC;
        a.outf = hdecf_cur; a.outf_k0 = 0;
        a.cell = d->c_dec; a.ldc = HDEC;
        MARK();
        TTS_HIP(sgemm_launch(a, ROLE_DEC_LSTM, s));
    }
    // 6) fused: mel = linear_projection([h_dec | ctx]) (tacotron2.py:214-217) -> history;
    //    prenet L1 of the next step; stop = sigmoid(stopnet([h_dec; mel])) + stop rule (:219-277)
    {
        SGemmArgs a = g;
        a.seg[0] = Seg{h_dec_cur, HDEC, HDEC, hdecf_cur};
        a.seg[1] = Seg{ctx_cur, XA, ENC, ctxf_cur};
        a.nseg = 2;
        a.W = d->W_melf; a.K = HDEC + ENC; a.N = nmel + PRE + 1; a.bias = d->b_melf;
        a.hist = d->mel_hist; a.ldh = (int64_t)d->hist_cap * nmel; a.hist_cap = d->hist_cap;
        MelFused& m = a.mf;
        m.nmel = nmel; m.pre1 = d->pre1; m.ldp = PRE;
        m.pre1f = fr ? d->pre1f : nullptr;
        m.stop_hist = d->stop_hist; m.stop_ldb = d->hist_cap;
        m.lens = d->lens; m.tail = d->tail; m.flag1 = d->flag1; m.count = d->count;
        m.done = d->done; m.n_steps = d->n_steps;
        m.state_next = d->state + 2 * q;
        m.stop_acc = d->state + 4;
        m.max_steps = max_steps;
        m.rule = rule;
        MARK();
        TTS_HIP(sgemm_launch(a, ROLE_MEL_FUSED, s));
    }
    MARK();
#undef MARK
    return TTS_OK;
}

// Step-0 prenet layer 1 on the go frame (later steps get it from the fused mel launch; under
// teacher forcing every step runs it on the teacher frame in mem, `slot` = that step's state slot).
tts_status enqueue_prenet_go(tts_decoder* d, int B, hipStream_t s, int* slot = nullptr) {
    SGemmArgs a{};
    a.B = B;
    a.step = slot ? slot : d->state;
    a.out_par = -1;
    a.seg[0] = Seg{d->mem, d->nmel, d->nmel};
    a.nseg = 1;
    a.W = d->W_pre1; a.K = d->nmel; a.N = PRE; a.act = ACT_RELU; a.bias = d->b_pre1;
    a.out = d->pre1; a.ldo = PRE;
    if (frag_on(d, B)) { a.outf = d->pre1f; a.outf_k0 = 0; a.ntf = d->ntf; }
    TTS_HIP(sgemm_launch(a, ROLE_PRENET, s));
    return TTS_OK;
}

InitArgs make_init_args(const tts_decoder* d, int B, const int* lens_dev) {
    InitArgs ia{};
    ia.B = B; ia.Lcap = d->Lcap; ia.nmel = d->nmel; ia.lens = lens_dev;
    ia.att_init = d->att_init; ia.dec_init = d->dec_init; ia.go = d->go;
    ia.h_att = d->h_att; ia.h_pstride = (int64_t)d->Bcap * HATT; ia.c_att = d->c_att;
    ia.h_dec = d->h_dec; ia.c_dec = d->c_dec; ia.xa = d->xa; ia.xa_pstride = (int64_t)d->Bcap * XA; ia.mem = d->mem;
    ia.alpha = d->alpha; ia.att_w = d->att_w; ia.att_cum = d->att_cum; ia.u = d->u; ia.win_idx = d->win_idx;
    ia.locf = d->locf;
    ia.nidx = d->nidx; ia.tail = d->tail; ia.flag1 = d->flag1; ia.count = d->count; ia.done = d->done; ia.n_steps = d->n_steps;
    ia.step = d->state; ia.n_active = d->state + 1;
    return ia;
}

// ---- tts_decoder_create: weight lookup, packing, resident setup, workspace ----

// The checkpoint tensors the decoder reads (device pointers the caller owns).
struct SrcWeights {
    const float *pre0, *pre1, *a_wih, *a_whh, *a_bih, *a_bhh, *wq, *win, *vw, *vb;
    const float *d_wih, *d_whh, *d_bih, *d_bhh, *pw, *pb, *sw, *sb, *ainit, *goinit, *dinit;
    const float *taw = nullptr, *tab = nullptr, *lcw = nullptr, *ldw = nullptr;
    const float *w_p0, *w_p1;  // the prenet weights every consumer packs: pre0 / pre1, or their BatchNorm folds
};

tts_status lookup_weights(const tts_decoder* d, const WeightMap& wm, SrcWeights& w) {
    const int nmel = d->nmel;
#define GW(var, key, n) \
    if (!(w.var = wm.get(key, n))) return TTS_ERR_INVALID;
    GW(pre0, "decoder.prenet.layers.0.linear_layer.weight", (int64_t)PRE * nmel);
    GW(pre1, "decoder.prenet.layers.1.linear_layer.weight", (int64_t)PRE * PRE);
    GW(a_wih, "decoder.attention_rnn.weight_ih", (int64_t)4 * HATT * XA);
    GW(a_whh, "decoder.attention_rnn.weight_hh", (int64_t)4 * HATT * HATT);
    GW(a_bih, "decoder.attention_rnn.bias_ih", 4 * HATT);
    GW(a_bhh, "decoder.attention_rnn.bias_hh", 4 * HATT);
    GW(wq, "decoder.attention_layer.query_layer.linear_layer.weight", (int64_t)ADIM * HATT);
    GW(win, "decoder.attention_layer.inputs_layer.linear_layer.weight", (int64_t)ADIM * ENC);
    GW(vw, "decoder.attention_layer.v.linear_layer.weight", ADIM);
    GW(vb, "decoder.attention_layer.v.linear_layer.bias", 1);
    GW(d_wih, "decoder.decoder_rnn.weight_ih", (int64_t)4 * HDEC * (HATT + ENC));
    GW(d_whh, "decoder.decoder_rnn.weight_hh", (int64_t)4 * HDEC * HDEC);
    GW(d_bih, "decoder.decoder_rnn.bias_ih", 4 * HDEC);
    GW(d_bhh, "decoder.decoder_rnn.bias_hh", 4 * HDEC);
    GW(pw, "decoder.linear_projection.linear_layer.weight", (int64_t)nmel * (HDEC + ENC));
    GW(pb, "decoder.linear_projection.linear_layer.bias", nmel);
    GW(sw, "decoder.stopnet.1.linear_layer.weight", HDEC + nmel);
    GW(sb, "decoder.stopnet.1.linear_layer.bias", 1);
    GW(ainit, "decoder.attention_rnn_init.weight", HATT);
    GW(goinit, "decoder.go_frame_init.weight", nmel);
    GW(dinit, "decoder.decoder_rnn_inits.weight", HDEC);
#undef GW
    if (d->cfg.trans_agent) {
        w.taw = wm.get("decoder.attention_layer.ta.weight", HATT + ENC);
        w.tab = wm.get("decoder.attention_layer.ta.bias", 1);
        if (!w.taw || !w.tab) return TTS_ERR_INVALID;
    }
    if (d->cfg.location_attn) {
        w.lcw = wm.get("decoder.attention_layer.location_layer.location_conv.weight", NLOC * 2 * KLOC);
        w.ldw = wm.get("decoder.attention_layer.location_layer.location_dense.linear_layer.weight", ADIM * NLOC);
        if (!w.lcw || !w.ldw) return TTS_ERR_INVALID;
    }
    w.w_p0 = w.pre0;
    w.w_p1 = w.pre1;
    return TTS_OK;
}

// the GEN_* bits (resident.h) of an attention configuration
int gen_bits(const tts_decoder_config& c) {
    return GEN_ON | (c.attn_norm == 0 ? GEN_SOFTMAX : 0) | (c.forward_attn ? GEN_FORWARD : 0) |
           (c.forward_attn && c.forward_attn_mask ? GEN_MASK : 0) | (c.forward_attn && c.trans_agent ? GEN_TA : 0) |
           (c.location_attn ? GEN_LOCATION : 0) | (c.windowing ? GEN_WINDOW : 0);
}

// Which attention launch and which resident form the configuration gets.
void choose_attention_form(tts_decoder* d) {
    const tts_decoder_config& c = d->cfg;
    AttnArgs probe{};
    probe.attn_norm = c.attn_norm; probe.forward_attn = c.forward_attn; probe.trans_agent = c.trans_agent;
    probe.forward_attn_mask = c.forward_attn_mask; probe.location_attn = c.location_attn;
    probe.windowing = c.windowing;
    probe.enc_dim = ENC;
    d->fast_attention = attention_uses_epart(probe);
    // the general resident form for every other configuration (resident.h); TTS_RESIDENT_GEN=0
    // keeps those on the multi-launch path (A/B, parity reference)
    if (!d->fast_attention && !env_is("TTS_RESIDENT_GEN", '0')) d->res_gen = gen_bits(c);
}

// prenet_type "bn" (common_layers.py:55-70, Decoder's Prenet(bias=False) layers/tacotron2.py:114):
// each layer is Linear -> BatchNorm1d (eval: running statistics, eps 1e-5) -> ReLU, folded here
// into the layer's weight plus a bias that every prenet consumer adds
tts_status fold_prenet_bn(tts_decoder* d, const WeightMap& wm, SrcWeights& w, hipStream_t s) {
    if (!wm.m.count("decoder.prenet.layers.0.bn.weight") && !wm.m.count("decoder.prenet.layers.1.bn.weight"))
        return TTS_OK;
    const int fan_in[2] = {d->nmel, PRE};
    const float* w_in[2] = {w.pre0, w.pre1};
    float* w_out[2] = {nullptr, nullptr};
    float* b_out[2] = {nullptr, nullptr};
    for (int l = 0; l < 2; ++l) {
        const std::string k = "decoder.prenet.layers." + std::to_string(l) + ".bn.";
        const float* g = wm.get(k + "weight", PRE);
        const float* be = wm.get(k + "bias", PRE);
        const float* mu = wm.get(k + "running_mean", PRE);
        const float* var = wm.get(k + "running_var", PRE);
        if (!g || !be || !mu || !var) return TTS_ERR_INVALID;
        TTS_TRY(d->dev.alloc(&w_out[l], (size_t)PRE * fan_in[l]));
        TTS_TRY(d->dev.alloc(&b_out[l], PRE));
        TTS_HIP(fold_linear_bn(w_in[l], nullptr, g, be, mu, var, PRE, fan_in[l], 1e-5f, w_out[l], b_out[l], s));
    }
    w.w_p0 = w_out[0]; w.w_p1 = w_out[1];
    d->b_pre1 = b_out[0]; d->b_pre2 = b_out[1];
    return TTS_OK;
}

// The resident decoder needs one workgroup per CU on >= 256 CUs and one mel row per CU;
// TTS_RESIDENT=0 disables it (multi-launch path for every batch).
void choose_resident(tts_decoder* d) {
    int dev = 0, ncu = 0, rate_khz = 0;
    if ((d->fast_attention || d->res_gen) && d->nmel <= RES_CUS && !env_is("TTS_RESIDENT", '0') &&
        hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu >= RES_CUS &&
        hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && rate_khz > 0 &&
        resident_prepare() == hipSuccess) {
        d->resident = true;
        d->res_ticks = (long long)rate_khz * 50;  // 50 ms per hand-off wait
        // fault injection for the timeout fallback test (TTS_DEC_WAIT_TICKS wall-clock ticks)
        if (const char* tk = getenv("TTS_DEC_WAIT_TICKS"); tk && tk[0]) d->res_ticks = std::max(1LL, atoll(tk));
    }
}

// The resident decoders' weight layouts: batch 1 (resident.h) and, for small batches of every
// attention configuration, the batched form with both LSTMs' rows in registers
// (TTS_RESIDENT_BATCH=0 keeps those multi-launch).  wf / bf: the folded mel matrix and bias.
tts_status pack_resident(tts_decoder* d, const SrcWeights& w, const float* wf, const float* bf, int nfused,
                         hipStream_t s) {
    size_t nwa, nwdl, nwdc;
    resident_weight_floats(&nwa, &nwdl, &nwdc);
    float *pa = nullptr, *pdl = nullptr, *pdc = nullptr;
    TTS_TRY(d->dev.alloc(&pa, nwa));
    TTS_TRY(d->dev.alloc(&pdl, nwdl));
    TTS_TRY(d->dev.alloc(&pdc, nwdc));
    TTS_TRY(d->dev.alloc(&d->rw.wf, (size_t)nfused * (HDEC + ENC)));
    TTS_TRY(d->dev.alloc(&d->rw.bf, nfused));
    TTS_TRY(d->dev.alloc(&d->rw.ba, RES_CUS * 16));
    TTS_TRY(d->dev.alloc(&d->rw.bd, RES_CUS * 16));
    TTS_TRY(d->dev.alloc(&d->rw.w2, (size_t)PRE * PRE));
    TTS_TRY(d->dev.alloc(&d->rw.b2, PRE));
    TTS_TRY(d->dev.alloc(&d->rw.wq, (size_t)ADIM * HATT));
    TTS_TRY(d->dev.alloc(&d->gran, (size_t)2 * GR_TOTAL + 2));
    d->rw.wa = reinterpret_cast<float4*>(pa);
    d->rw.wdl = reinterpret_cast<float4*>(pdl);
    d->rw.wdc = reinterpret_cast<float4*>(pdc);
    ResSrc src{w.a_wih, w.a_whh, w.a_bih, w.a_bhh, w.d_wih, w.d_whh, w.d_bih, w.d_bhh, w.w_p1, d->b_pre2, w.wq, wf, bf,
               nfused};
    TTS_HIP(resident_pack(src, d->rw, s));
    const int gen = gen_bits(d->cfg);
    // location features / windowing / transition agent run the general instantiations, which need
    // the general batch-1 form's packed location weights (res_gen); TTS_RB_GENERAL=0 keeps those
    // configurations on the routing without them (serial batch-1 calls or multi-launch; A/B, tests)
    if (resident_batch_general(gen) && (!d->res_gen || env_is("TTS_RB_GENERAL", '0'))) return TTS_OK;
    if (!(d->cfg.max_batch >= 2 && resident_batch_supports(gen) && !env_is("TTS_RESIDENT_BATCH", '0') &&
          resident_batch_prepare() == hipSuccess))
        return TTS_OK;
    size_t nra, nrd;
    resident_batch_weight_floats(&nra, &nrd);
    float *qa = nullptr, *qd = nullptr;
    TTS_TRY(d->dev.alloc(&qa, nra));
    TTS_TRY(d->dev.alloc(&qd, nrd));
    TTS_TRY(d->dev.alloc(&d->rb_gran, resident_batch_granules() + 2));
    d->rb_wa = reinterpret_cast<float4*>(qa);
    d->rb_wd = reinterpret_cast<float4*>(qd);
    TTS_HIP(resident_batch_pack(src, d->rb_wa, d->rb_wd, s));
    TTS_HIP(hipMemsetAsync(d->rb_gran, 0, sizeof(unsigned long long) * (resident_batch_granules() + 2), s));
    d->rbatch = true;
    d->rb_gen = gen;
    return TTS_OK;
}

// The fused [mel | next prenet L1 | stopnet] matrix from its folded logical form wf / bf
// (temporaries of create_weights), then the resident layouts that read the same fold.
tts_status pack_mel_fused(tts_decoder* d, const SrcWeights& w, float* wf, float* bf, int nfused, hipStream_t s) {
    const int nmel = d->nmel;
    TTS_HIP(fold_mel_weights(w.pw, w.pb, w.w_p0, d->b_pre1, w.sw, w.sb, nmel, HDEC + ENC, HDEC, wf, bf, s));
    TTS_TRY(pack_linear(d->dev, wf, nfused, HDEC + ENC, &d->W_melf, s));
    TTS_TRY(pack_bias(d->dev, bf, nullptr, nfused, ROWMAP_IDENTITY, 0, &d->b_melf, s));
    if (d->resident) TTS_TRY(pack_resident(d, w, wf, bf, nfused, s));
    return TTS_OK;
}

tts_status create_weights(tts_decoder* d, const WeightMap& wm, SrcWeights& w, hipStream_t s) {
    const int nmel = d->nmel;
    choose_attention_form(d);
    TTS_TRY(fold_prenet_bn(d, wm, w, s));
    choose_resident(d);
    // packed GEMM weights
    TTS_TRY(pack_linear(d->dev, w.w_p0, PRE, nmel, &d->W_pre1, s));
    TTS_TRY(pack_linear(d->dev, w.w_p1, PRE, PRE, &d->W_pre2, s));
    TTS_TRY(d->dev.alloc(&d->W_att, sgemm_packed_floats(4 * HATT, XA + HATT)));
    TTS_HIP(sgemm_pack(w.a_wih, XA, w.a_whh, HATT, 4 * HATT, ROWMAP_LSTM, HATT, d->W_att, s));
    TTS_TRY(pack_bias(d->dev, w.a_bih, w.a_bhh, 4 * HATT, ROWMAP_LSTM, HATT, &d->b_att, s));
    TTS_TRY(pack_linear(d->dev, w.wq, ADIM, HATT, &d->W_q, s));
    TTS_TRY(d->dev.alloc(&d->W_dec, sgemm_packed_floats(4 * HDEC, HATT + ENC + HDEC)));
    TTS_HIP(sgemm_pack(w.d_wih, HATT + ENC, w.d_whh, HDEC, 4 * HDEC, ROWMAP_LSTM, HDEC, d->W_dec, s));
    TTS_TRY(pack_bias(d->dev, w.d_bih, w.d_bhh, 4 * HDEC, ROWMAP_LSTM, HDEC, &d->b_dec, s));
    {
        // the folded logical matrix is a temporary: one synchronisation, after everything that reads
        // it is enqueued, then it is freed (on an error too)
        const int nfused = nmel + PRE + 1;
        float *wf = nullptr, *bf = nullptr;
        TTS_HIP(hipMalloc(&wf, sizeof(float) * nfused * (HDEC + ENC)));
        TTS_HIP(hipMalloc(&bf, sizeof(float) * nfused));
        tts_status st = pack_mel_fused(d, w, wf, bf, nfused, s);
        const hipError_t e = st ? hipSuccess : hipStreamSynchronize(s);
        (void)hipFree(wf);
        (void)hipFree(bf);
        if (st) return st;
        TTS_HIP(e);
    }
    // small weights in reference layout
    TTS_TRY(copy_weight(d->dev, &d->v, w.vw, ADIM, s));
    TTS_TRY(copy_weight(d->dev, &d->v_b, w.vb, 1, s));
    TTS_TRY(copy_weight(d->dev, &d->W_in, w.win, (size_t)ADIM * ENC, s));
    TTS_TRY(copy_weight(d->dev, &d->att_init, w.ainit, HATT, s));
    TTS_TRY(copy_weight(d->dev, &d->dec_init, w.dinit, HDEC, s));
    TTS_TRY(copy_weight(d->dev, &d->go, w.goinit, nmel, s));
    if (w.taw) {
        TTS_TRY(copy_weight(d->dev, &d->ta_w, w.taw, HATT + ENC, s));
        TTS_TRY(copy_weight(d->dev, &d->ta_b, w.tab, 1, s));
    }
    if (w.lcw) {
        TTS_TRY(copy_weight(d->dev, &d->loc_conv, w.lcw, NLOC * 2 * KLOC, s));
        TTS_TRY(copy_weight(d->dev, &d->loc_dense, w.ldw, ADIM * NLOC, s));
        if (d->resident && d->res_gen) {
            TTS_TRY(d->dev.alloc(&d->loc_conv_p, 2 * NLOC * 32));
            TTS_HIP(resident_pack_location(d->loc_conv, d->loc_conv_p, s));
        }
        if (d->rbatch && resident_batch_general(d->rb_gen)) {
            TTS_TRY(d->dev.alloc(&d->rb_loc, RB_LOC_FLOATS));
            TTS_HIP(resident_batch_pack_location(d->loc_conv, d->loc_dense, d->rb_loc, s));
        }
    }
    return TTS_OK;
}

tts_status create_workspace(tts_decoder* d, hipStream_t s) {
    const tts_decoder_config& cfg = d->cfg;
    const int nmel = d->nmel;
    const int Bc = cfg.max_batch, Lc = (cfg.max_len + 3) / 4 * 4;
    d->Bcap = Bc;
    d->Lcap = Lc;
    d->hist_cap = cfg.max_steps + 21;
    TTS_TRY(d->dev.alloc(&d->enc, (size_t)Bc * Lc * ENC));
    TTS_TRY(d->dev.alloc(&d->Pt, (size_t)Bc * ADIM * Lc));
    TTS_TRY(d->dev.alloc(&d->h_att, (size_t)2 * Bc * HATT));
    TTS_TRY(d->dev.alloc(&d->c_att, (size_t)Bc * HATT));
    TTS_TRY(d->dev.alloc(&d->h_dec, (size_t)2 * Bc * HDEC));
    TTS_TRY(d->dev.alloc(&d->c_dec, (size_t)Bc * HDEC));
    TTS_TRY(d->dev.alloc(&d->xa, (size_t)2 * Bc * XA));
    TTS_TRY(d->dev.alloc(&d->mem, (size_t)Bc * nmel));
    TTS_TRY(d->dev.alloc(&d->pre1, (size_t)Bc * PRE));
    TTS_TRY(d->dev.alloc(&d->pre1_go, (size_t)PRE));
    TTS_TRY(d->dev.alloc(&d->q, (size_t)Bc * ADIM));
    if (Bc > 16) {
        d->ntf = (Bc + 15) / 16;
        const size_t rows = (size_t)d->ntf * 16;
        // three m-tiles run the four-tile kernel (sgemm.hip: launch_role): at ntf == 3 its fourth
        // tile of chunk c is tile 0 of chunk c + 1, one tile (256 floats) past the mirror at the
        // last chunk.  The rows of that tile are never stored; the slack keeps the read in bounds.
        const size_t slack = d->ntf == 3 ? 256 : 0;
        TTS_TRY(d->dev.alloc(&d->xaf, 2 * rows * XA + slack));
        TTS_TRY(d->dev.alloc(&d->hattf, 2 * rows * HATT + slack));
        TTS_TRY(d->dev.alloc(&d->hdecf, 2 * rows * HDEC + slack));
        TTS_TRY(d->dev.alloc(&d->pre1f, rows * PRE + slack));
    }
    TTS_TRY(d->dev.alloc(&d->epart, (size_t)Bc * QE_TILES * Lc));
    if (cfg.location_attn) TTS_TRY(d->dev.alloc(&d->locf, (size_t)Bc * NLOC * Lc));
    // alpha / att_cum / win_idx / nidx: two parity slots (the split general attention launch reads
    // slot t & 1 and writes the other; the fast paths use slot 0 only)
    TTS_TRY(d->dev.alloc(&d->alpha, (size_t)2 * Bc * Lc));
    TTS_TRY(d->dev.alloc(&d->att_w, (size_t)Bc * Lc));
    TTS_TRY(d->dev.alloc(&d->att_cum, (size_t)2 * Bc * Lc));
    TTS_TRY(d->dev.alloc(&d->u, Bc));
    TTS_TRY(d->dev.alloc(&d->tail, Bc));
    TTS_TRY(d->dev.alloc(&d->lens, Bc));
    TTS_TRY(d->dev.alloc(&d->win_idx, 2 * Bc));
    TTS_TRY(d->dev.alloc(&d->nidx, 2 * Bc));
    TTS_TRY(d->dev.alloc(&d->flag1, Bc));
    TTS_TRY(d->dev.alloc(&d->count, Bc));
    TTS_TRY(d->dev.alloc(&d->done, Bc));
    TTS_TRY(d->dev.alloc(&d->n_steps, Bc));
    TTS_TRY(d->dev.alloc(&d->state, 8));  // {step, n_active} x 2 parities (kernels load one slot as int2), stop_acc
    TTS_TRY(d->dev.alloc(&d->mel_hist, (size_t)Bc * d->hist_cap * nmel));
    TTS_TRY(d->dev.alloc(&d->stop_hist, (size_t)Bc * d->hist_cap));
    TTS_TRY(d->dev.alloc(&d->align_hist, (size_t)Bc * d->hist_cap * Lc));
    TTS_HIP(attention_prepare(Lc, cfg.location_attn));
    TTS_HIP(hipMemsetAsync(d->xa, 0, sizeof(float) * 2 * Bc * XA, s));
    TTS_HIP(hipMemsetAsync(d->h_att, 0, sizeof(float) * 2 * Bc * HATT, s));
    TTS_HIP(hipMemsetAsync(d->h_dec, 0, sizeof(float) * 2 * Bc * HDEC, s));
    TTS_HIP(hipMemsetAsync(d->mem, 0, sizeof(float) * Bc * nmel, s));
    TTS_HIP(hipMemsetAsync(d->enc, 0, sizeof(float) * Bc * Lc * ENC, s));
    TTS_HIP(hipMemsetAsync(d->Pt, 0, sizeof(float) * Bc * ADIM * Lc, s));
    TTS_HIP(hipMemsetAsync(d->state, 0, sizeof(int) * 8, s));
    TTS_HIP(hipStreamSynchronize(s));
    return TTS_OK;
}

// ---- decoder_run: staging, the three ways to run the steps, copy-out ----

// What the stages of one decoder_run share; the driver builds it on its stack.
struct RunCtx {
    const float* enc;     // caller's encoder output [B][Lmax][ENC]
    const int32_t* lens;  // host lengths
    int32_t* n_steps;     // host step counts (out)
    int B, Lmax, max_steps;
    hipStream_t s;
    InitArgs ia;
    bool direct;  // a fresh batch-1 resident run reading the caller's buffers in place (stage_inputs)
    bool keep;    // tts_decoder_run_continue: RNN states, context and memory carry over
    bool timed;   // stage timers (tts_decoder_last_timing)
    int first;    // steps of the first chunk: the reference's lower bound on the step count
    int run;      // steps enqueued; the next step has parity run & 1
};

bool verbose() {
    static const bool v = env_is("TTS_VERBOSE", '1');
    return v;
}

tts_status stage_encoder(tts_decoder* d, const RunCtx& c) {
    TTS_HIP(hipMemcpy2DAsync(d->enc, (size_t)d->Lcap * ENC * 4, c.enc, (size_t)c.Lmax * ENC * 4, (size_t)c.Lmax * ENC * 4,
                             c.B, hipMemcpyDeviceToDevice, c.s));
    return TTS_OK;
}

// Lengths, the first chunk, the hand-over from the caller's stream `cs`, the encoder output and its
// projection, the initial state (or the carried one) and the go frame's prenet layer 1.
tts_status stage_inputs(tts_decoder* d, RunCtx& c, hipStream_t cs) {
    const int B = c.B;
    hipStream_t s = c.s;
    c.first = 0;
    for (int b = 0; b < B; ++b) {
        TTS_CHECK(c.lens[b] >= 2 && c.lens[b] <= c.Lmax, TTS_ERR_INVALID, "encoder length out of range [2, Lmax]");
        c.first = std::max(c.first, std::min(2 * c.lens[b] + 22, c.max_steps));
    }
    if (s != cs) {
        TTS_HIP(hipEventRecord(d->ev_in, cs));
        TTS_HIP(hipStreamWaitEvent(s, d->ev_in, 0));
    }
    // A fresh batch-1 resident run ("direct") reads the caller's encoder output in place, the length
    // from the pipeline's device array when it has one, zeroes its hand-off granules and takes the
    // cached go-frame prenet row inside decoder_init: two launches before the resident one instead
    // of six.  A fallback to the multi-launch path stages the copies first (restart_multilaunch).
    c.direct = d->resident && B == 1 && c.lens[0] <= RES_LMAX && !c.keep;
    if (!c.direct) TTS_TRY(stage_encoder(d, c));
    const int* lens_dev = c.direct && d->io_lens ? d->io_lens : d->lens;
    if (lens_dev == d->lens) TTS_HIP(hipMemcpyAsync(d->lens, c.lens, sizeof(int) * B, hipMemcpyHostToDevice, s));
    // (the memory projection goes out with the init launch below, unless the VALU form is asked for)
    static const bool proj_valu = env_is("TTS_PROJ_VALU", '1');  // measurement: the VALU projection launch
    const float* enc_in = c.direct ? c.enc : d->enc;
    if (proj_valu) TTS_HIP(launch_project_inputs(enc_in, d->W_in, B, c.Lmax, d->Lcap, d->Pt, s));
    d->last_enc_direct = c.direct ? c.enc : nullptr;
    d->last_len_direct = c.lens[0];
    InitArgs& ia = c.ia;
    ia = make_init_args(d, B, lens_dev);
    if (c.keep) {
        // Decoder.inference_truncated (layers/tacotron2.py:287-328): attention / stop state restart,
        // the RNN states, context and memory (the last mel frame) carry over.  The last step of the
        // previous run (parity (n-1) & 1) left h_att / h_dec in its slot, the context in the other
        // parity's xa row, and relu(W1 mel_last) in pre1 (the fused mel launch computes the next
        // step's prenet layer 1): move them to the slots step 0 reads.
        const int pl = (d->last_steps_done - 1) & 1;
        const size_t hp = (size_t)d->Bcap * HATT;
        if (pl != 1) {
            TTS_HIP(hipMemcpyAsync(d->h_att + hp, d->h_att, HATT * sizeof(float), hipMemcpyDeviceToDevice, s));
            TTS_HIP(hipMemcpyAsync(d->h_dec + hp, d->h_dec, HDEC * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        if (1 - pl != 0)
            TTS_HIP(hipMemcpyAsync(d->xa + PRE, d->xa + (size_t)d->Bcap * XA + PRE, ENC * sizeof(float),
                                   hipMemcpyDeviceToDevice, s));
        ia.keep = 1;
    }
    if (c.direct) {
        ia.zero = d->gran;
        ia.nzero = 2 * GR_TOTAL + 2;
        ia.pre1 = d->pre1;
        ia.pre1_go = d->pre1_go_ok ? d->pre1_go : nullptr;
    }
    if (!proj_valu) TTS_HIP(launch_project_init(enc_in, d->W_in, B, c.Lmax, d->Lcap, d->Pt, ia, s));
    else TTS_HIP(launch_decoder_init(ia, s));
    if (frag_on(d, B)) TTS_TRY(enqueue_frag_sync(d, B, s));
    if (!c.keep && !ia.pre1_go) {
        TTS_TRY(enqueue_prenet_go(d, B, s));
        if (c.direct) {
            TTS_HIP(hipMemcpyAsync(d->pre1_go, d->pre1, PRE * sizeof(float), hipMemcpyDeviceToDevice, s));
            d->pre1_go_ok = true;
        }
    }
    return TTS_OK;
}

// Start this batch again, from its initial state, on the multi-launch path: after a resident launch
// that did not run (co-residency, placement) or gave up (hand-off timeout).  A direct run first
// stages the inputs the step graphs read.
tts_status restart_multilaunch(tts_decoder* d, RunCtx& c) {
    InitArgs& ia = c.ia;
    if (c.direct) {
        TTS_TRY(stage_encoder(d, c));
        if (ia.lens != d->lens) TTS_HIP(hipMemcpyAsync(d->lens, c.lens, sizeof(int) * c.B, hipMemcpyHostToDevice, c.s));
        ia.lens = d->lens;
        ia.zero = nullptr;
        ia.nzero = 0;
        ia.pre1_go = nullptr;
        d->last_enc_direct = nullptr;
    }
    TTS_HIP(launch_decoder_init(ia, c.s));
    if (frag_on(d, c.B)) TTS_TRY(enqueue_frag_sync(d, c.B, c.s));
    if (!c.keep) TTS_TRY(enqueue_prenet_go(d, c.B, c.s));
    return TTS_OK;
}

// Launch arguments of the batched resident decoder for sentences [g0, g0 + nb): each sentence's
// state, histories and step count in the multi-launch path's slots.
void fill_batch_args(const tts_decoder* d, const RunCtx& c, int g0, int nb, ResBatchArgs& rb) {
    rb.B = nb;
    rb.gen = d->rb_gen;
    for (int b = 0; b < nb; ++b) rb.L[b] = c.lens[g0 + b];
    rb.Lcap = d->Lcap; rb.nmel = d->nmel; rb.nrows = d->nmel + PRE + 1; rb.max_steps = c.max_steps;
    rb.hist_cap = d->hist_cap; rb.Lalign = c.Lmax; rb.timeout_ticks = d->res_ticks;
    rb.wa = d->rb_wa; rb.wd = d->rb_wd;
    rb.w2 = d->rw.w2; rb.b2 = d->rw.b2; rb.wq = d->rw.wq; rb.wf = d->rw.wf; rb.bf = d->rw.bf; rb.ba = d->rw.ba;
    rb.bd = d->rw.bd;
    rb.v = d->v; rb.v_b = d->v_b;
    rb.Pt = d->Pt + (size_t)g0 * ADIM * d->Lcap;
    rb.enc = d->enc + (size_t)g0 * d->Lcap * ENC;
    rb.h_att = d->h_att + (size_t)g0 * HATT; rb.c_att = d->c_att + (size_t)g0 * HATT;
    rb.h_dec = d->h_dec + (size_t)g0 * HDEC; rb.c_dec = d->c_dec + (size_t)g0 * HDEC;
    rb.xa = d->xa + (size_t)g0 * XA;
    rb.hps = (int64_t)d->Bcap * HATT; rb.xps = (int64_t)d->Bcap * XA;
    rb.pre1 = d->pre1 + (size_t)g0 * PRE;
    rb.alpha = d->alpha + (size_t)g0 * d->Lcap;
    rb.nidx = d->nidx + g0; rb.u = d->u + g0; rb.flag1 = d->flag1 + g0; rb.count = d->count + g0;
    rb.done = d->done + g0; rb.n_steps = d->n_steps + g0;
    rb.mel_hist = d->mel_hist + (size_t)g0 * d->hist_cap * d->nmel;
    rb.stop_hist = d->stop_hist + (size_t)g0 * d->hist_cap;
    rb.align_hist = d->align_hist + (size_t)g0 * d->hist_cap * c.Lmax;
    rb.ta_w = d->ta_w; rb.ta_b = d->ta_b;
    rb.att_w0 = d->att_w + (size_t)g0 * d->Lcap; rb.att_cum0 = d->att_cum + (size_t)g0 * d->Lcap;
    rb.win0 = d->win_idx + g0;
    rb.loc_conv = d->rb_loc; rb.loc_dense = d->rb_loc ? d->rb_loc + RB_LOC_CONV_FLOATS : nullptr;
    rb.gran = d->rb_gran;
    static const int rb_hatt = env_int("TTS_RB_SLEEP_HATT", 0), rb_hdec = env_int("TTS_RB_SLEEP_HDEC", 0),
                     rb_pre2 = env_int("TTS_RB_SLEEP_PRE2", 0), rb_ctx = env_int("TTS_RB_SLEEP_CTX", 0);
    rb.sleep_hatt = rb_hatt; rb.sleep_hdec = rb_hdec; rb.sleep_pre2 = rb_pre2; rb.sleep_ctx = rb_ctx;
    rb.status = reinterpret_cast<int*>(d->rb_gran + resident_batch_granules());
}

// TTS_RB_PROF=1: microseconds per step of each phase (wall clock 100 MHz) for every wave index:
// min / mean / max over the 256 CUs; then, for one step (RB_PROF_T), the last publisher of an edge
// against each CU's arrival.
tts_status report_rb_prof(const long long* prof, int nb) {
    std::vector<long long> pk((size_t)RES_CUS * 4 * RB_PROF_SLOTS);
    TTS_HIP(hipMemcpy(pk.data(), prof, pk.size() * sizeof(long long), hipMemcpyDeviceToHost));
    auto at = [&](int cu, int w, int k) { return pk[((size_t)cu * 4 + w) * RB_PROF_SLOTS + k]; };
    const double steps = pk[RB_PROF_SLOTS - 1] > 0 ? (double)pk[RB_PROF_SLOTS - 1] : 1.0;
    fprintf(stderr, "[tts] resident batch nb=%d steps=%lld (us/step per phase: min/mean/max over CUs)\n", nb,
            pk[RB_PROF_SLOTS - 1]);
    for (int w = 0; w < 4; ++w) {
        fprintf(stderr, "[tts]  wave %d:", w);
        for (int k : {0, 1, 2, 3, 4, 5, 6, 20, 21, 22, 23, 7, 8, 9, 10, 19, 11, 12}) {
            double mn = 1e30, mx = 0, sum = 0;
            for (int cu = 0; cu < RES_CUS; ++cu) {
                const double v = at(cu, w, k) * 0.01 / steps;
                mn = std::min(mn, v);
                mx = std::max(mx, v);
                sum += v;
            }
            fprintf(stderr, " %d:%.2f/%.2f/%.2f", k, mn, sum / RES_CUS, mx);
        }
        fprintf(stderr, "\n");
    }
    if (pk[RB_PROF_SLOTS - 1] <= RB_PROF_T) return TTS_OK;
    const char* names[] = {"h_att", "h_dec"};
    const int pubk[] = {13, 16}, donek[] = {14, 17};
    for (int e = 0; e < 2; ++e) {
        long long pmin = LLONG_MAX, pmax = 0, dmin = LLONG_MAX, dmax = 0;
        int pmax_cu = -1;
        for (int cu = 0; cu < RES_CUS; ++cu)
            for (int w = 0; w < 4; ++w) {
                const long long p = at(cu, w, pubk[e]), q = at(cu, w, donek[e]);
                if (p < pmin) pmin = p;
                if (p > pmax) { pmax = p; pmax_cu = cu * 4 + w; }
                dmin = std::min(dmin, q);
                dmax = std::max(dmax, q);
            }
        fprintf(stderr, "[tts]  step %d %s: publish spread %.2f us (last: CU %d wave %d), arrival after the last publish %.2f .. %.2f us\n",
                RB_PROF_T, names[e], (pmax - pmin) * 0.01, pmax_cu / 4, pmax_cu % 4, (dmin - pmax) * 0.01,
                (dmax - pmax) * 0.01);
    }
    return TTS_OK;
}

// Batches of 2..rb_max_batch() short sentences: one persistent launch per group of <= RB_MAXB
// sentences (resident_batch.hip).  Consecutive launches beat the multi-launch step (~45 us at any
// batch up to 64) only for a few groups: TTS_RB_MAX bounds the batch.  *served: every group ran to
// its end; otherwise the whole batch is back at its initial state for the multi-launch path.
tts_status run_resident_batch(tts_decoder* d, RunCtx& c, bool* served) {
    static const bool rb_prof = env_is("TTS_RB_PROF", '1');
    const int B = c.B;
    hipStream_t s = c.s;
    bool rb_ok = d->rbatch && B >= 2 && B <= rb_max_batch() && !c.keep;
    for (int b = 0; rb_ok && b < B; ++b) rb_ok = c.lens[b] <= RES_LMAX;
    if (!rb_ok) return TTS_OK;
    if (c.timed) TTS_HIP(hipEventRecord(d->ev_t0, s));
    bool all = true;
    for (int g0 = 0; g0 < B && all; g0 += RB_MAXB) {
        const int nb = std::min(RB_MAXB, B - g0);
        ResBatchArgs rb{};
        fill_batch_args(d, c, g0, nb, rb);
        if (rb_prof && !d->rb_prof) TTS_TRY(d->dev.alloc(&d->rb_prof, (size_t)RES_CUS * 4 * RB_PROF_SLOTS));
        rb.prof = rb_prof ? d->rb_prof : nullptr;
        bool wrapped = false;
        d->rb_salt = res_next_salt(d->rb_salt, &wrapped);
        rb.salt = d->rb_salt;
        if (wrapped)
            TTS_HIP(hipMemsetAsync(d->rb_gran, 0, sizeof(unsigned long long) * (resident_batch_granules() + 2), s));
        TTS_HIP(hipMemsetAsync(rb.status, 0, 4 * sizeof(int), s));
        bool launched = false;
        TTS_HIP(launch_resident_batch(rb, s, &launched));
        if (verbose()) fprintf(stderr, "[tts] resident batch launch g0=%d nb=%d launched=%d\n", g0, nb, (int)launched);
        if (!launched) {
            d->rbatch = false;  // the grid cannot be co-resident on this device
            all = false;
            break;
        }
        TTS_HIP(hipMemcpyAsync(d->host_flags, rb.status, sizeof(int), hipMemcpyDeviceToHost, s));
        TTS_HIP(hipMemcpyAsync(d->host_flags + 4 + g0, d->n_steps + g0, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
        TTS_HIP(spin_sync(s, d->ev_sync));
        if (verbose()) fprintf(stderr, "[tts] resident batch status=%d\n", d->host_flags[0]);
        if (d->host_flags[0] != 0) {
            TTS_CHECK(d->host_flags[0] != 100, TTS_ERR_HIP, "decoder did not stop within max_steps + 20 (internal error)");
            if (d->host_flags[0] == RES_STATUS_PLACEMENT) {
                if (++d->rb_place_fails >= RES_PLACEMENT_RETRIES) d->rbatch = false;
            } else {
                ++d->res_timeouts;
            }
            all = false;
            break;
        }
        d->rb_place_fails = 0;
        if (rb_prof) TTS_TRY(report_rb_prof(rb.prof, nb));
    }
    if (!all) return restart_multilaunch(d, c);
    if (c.timed) TTS_HIP(hipEventRecord(d->ev_t1, s));
    std::copy(d->host_flags + 4, d->host_flags + 4 + B, c.n_steps);
    c.run = 0;
    for (int b = 0; b < B; ++b) c.run = std::max(c.run, (int)c.n_steps[b]);
    d->last_resident = 2;
    *served = true;
    return TTS_OK;
}

// Launch arguments of the batch-1 resident decoder (resident.h): the multi-launch path's state and
// history buffers.
void fill_resident_args(const tts_decoder* d, const RunCtx& c, ResArgs& ra) {
    ra.w = d->rw;
    ra.L = c.lens[0]; ra.Lcap = d->Lcap; ra.nmel = d->nmel; ra.nrows = d->nmel + PRE + 1;
    ra.max_steps = c.max_steps; ra.hist_cap = d->hist_cap; ra.Lalign = c.Lmax; ra.timeout_ticks = d->res_ticks;
    ra.v = d->v; ra.v_b = d->v_b; ra.Pt = d->Pt; ra.enc = c.direct ? c.enc : d->enc;
    ra.h_att = d->h_att; ra.c_att = d->c_att; ra.h_dec = d->h_dec; ra.c_dec = d->c_dec; ra.xa = d->xa;
    ra.hps = (int64_t)d->Bcap * HATT; ra.xps = (int64_t)d->Bcap * XA;
    ra.pre1 = d->pre1; ra.alpha = d->alpha; ra.nidx = d->nidx; ra.u = d->u; ra.flag1 = d->flag1; ra.count = d->count;
    ra.done = d->done; ra.n_steps = d->n_steps;
    ra.mel_hist = d->mel_hist; ra.stop_hist = d->stop_hist; ra.align_hist = d->align_hist;
    ra.gen = d->res_gen;
    ra.ta_w = d->ta_w; ra.ta_b = d->ta_b; ra.att_w0 = d->att_w; ra.att_cum0 = d->att_cum; ra.win0 = d->win_idx;
    ra.loc_conv = d->loc_conv_p; ra.loc_dense = d->loc_dense;
    ra.gran = d->gran;
    // first-poll delays (resident.h; round 6: h_att 5 / h_dec 5 took a configs[1] sentence from
    // 2.65 to 2.29 ms, tools/cases_sleep.txt); TTS_RES_SLEEP_* override them (_Q: the synthesis
    // form's energy-partials gather and the general form's query gather; _CTX, _E: general form only)
    // The synthesis form's defaults are h_att 0 / h_dec 0: both LSTMs' recurrent partials run inside
    // those two waits (the decoder LSTM's ahead of the h_att poll, the attention LSTM's ahead of the
    // h_dec poll, beside the tail / alpha bookkeeping; the attention operand loads left the h_att
    // wait for the step's end, re-swept 0 / 1 / 2: profiles/r12_ab_parts.txt) and are the
    // first-poll delay themselves; any s_sleep on top of them lost (profiles/r11_looptop_parts.txt).
    // The general form keeps 5 / 5.
    static const int sl_hatt_env = env_int("TTS_RES_SLEEP_HATT", -1), sl_hdec_env = env_int("TTS_RES_SLEEP_HDEC", -1);
    const int sl_hatt = sl_hatt_env >= 0 ? sl_hatt_env : (d->res_gen ? 5 : 0),
              sl_hdec = sl_hdec_env >= 0 ? sl_hdec_env : (d->res_gen ? 5 : 0);
    static const int sl_p1 = env_int("TTS_RES_SLEEP_P1", 0), sl_pre2 = env_int("TTS_RES_SLEEP_PRE2", 2),
                     sl_ctx = env_int("TTS_RES_SLEEP_CTX", 0), sl_q = env_int("TTS_RES_SLEEP_Q", 0),
                     sl_e = env_int("TTS_RES_SLEEP_E", 0);
    ra.sleep_hatt = sl_hatt; ra.sleep_hdec = sl_hdec; ra.sleep_p1 = sl_p1; ra.sleep_pre2 = sl_pre2;
    ra.sleep_ctx = sl_ctx; ra.sleep_q = sl_q; ra.sleep_e = sl_e;
    ra.status = reinterpret_cast<int*>(d->gran + 2 * GR_TOTAL);
}

// Status, step counts (and the pipeline's extra word / GL clamp) in one launch, then the sequence
// word the host polls.
tts_status enqueue_readback(tts_decoder* d, const RunCtx& c, const int* status, int seq) {
    Readback rb{};
    rb.src[0] = status; rb.n[0] = 1; rb.dst[0] = d->host_flags;
    rb.src[1] = d->n_steps; rb.n[1] = c.B; rb.dst[1] = d->host_flags + 4;
    rb.count = 2;
    if (d->io_rb_src) { rb.src[2] = d->io_rb_src; rb.n[2] = 1; rb.dst[2] = d->io_rb_dst; rb.count = 3; }
    if (d->io_clamp) {
        rb.clamp_src = d->n_steps; rb.clamp_dst = d->io_clamp; rb.clamp_n = c.B; rb.clamp_max = d->io_clamp_max;
    }
    rb.seq_dst = d->host_flags + 3;
    rb.seq = seq;
    TTS_HIP(readback(rb, c.s));
    return TTS_OK;
}

// Batch 1, short sentence: one persistent launch runs every step (resident.h).  *served: it ran to
// its end; otherwise the sentence is back at its initial state for the multi-launch path.
tts_status run_resident_one(tts_decoder* d, RunCtx& c, bool* served) {
    if (!(d->resident && c.B == 1 && c.lens[0] <= RES_LMAX)) return TTS_OK;
    hipStream_t s = c.s;
    ResArgs ra{};
    fill_resident_args(d, c, ra);
    // direct (pipelined) runs skip the per-launch clear and rely on the 18-bit tag salt: on a
    // salt wrap a granule left 2^18 launches back could match a current wait, so clear then
    bool wrapped = false;
    d->res_salt = res_next_salt(d->res_salt, &wrapped);
    ra.salt = d->res_salt;
    d->last_ra = ra;
    if (!c.direct || wrapped)
        TTS_HIP(hipMemsetAsync(d->gran, 0, sizeof(unsigned long long) * (2 * GR_TOTAL + 2), s));
    if (c.timed) TTS_HIP(hipEventRecord(d->ev_t0, s));
    bool launched = false;
    TTS_HIP(launch_resident(ra, s, &launched));
    if (verbose()) fprintf(stderr, "[tts] resident launch: launched=%d\n", (int)launched);
    if (!launched) {
        // the grid cannot be co-resident on this device (launch_persistent): nothing ran and the
        // initial state is untouched; the multi-launch path takes over for the life of the handle
        d->resident = false;
        return restart_multilaunch(d, c);
    }
    if (c.timed) TTS_HIP(hipEventRecord(d->ev_t1, s));
    const int seq = ++d->rb_seq;
    TTS_TRY(enqueue_readback(d, c, ra.status, seq));
    // a polling wait on the read-back's sequence word (no event marker); work that needs no
    // host-side step count (the synthesis postnet, Griffin-Lim) is enqueued before it, so the
    // device does not idle while the host wakes
    if (d->post_hook) {
        d->post_hook(d->post_ctx, s);
        d->hook_ran = true;
    }
    TTS_HIP(spin_word(d->host_flags + 3, seq, s));
    const int status = d->host_flags[0];
    c.n_steps[0] = d->host_flags[4];
    if (verbose()) fprintf(stderr, "[tts] resident status=%d steps=%d\n", status, c.n_steps[0]);
    if (status == RES_STATUS_PLACEMENT) {
        // the runtime placed fewer than RES_MIN_CUS_PER_XCD workgroups on some XCD (or, for the
        // general form, more than that on one): the kernel stopped before touching any state.
        // This sentence runs multi-launch; the handle gives the resident path up only after
        // RES_PLACEMENT_RETRIES such sentences in a row (one uneven dispatch is not a device that
        // cannot place the grid: ADVICE r5)
        if (++d->res_place_fails >= RES_PLACEMENT_RETRIES) d->resident = false;
        if (verbose())
            fprintf(stderr, "[tts] resident decoder: placement failed (%d in a row)%s\n", d->res_place_fails,
                    d->resident ? "" : ", multi-launch from now on");
        return restart_multilaunch(d, c);
    }
    if (status != 0 && status != 100 && !c.keep) {
        // a hand-off wait timed out (a workgroup could not become resident beside another
        // stream's work, e.g. a pipelined Griffin-Lim): every wave drained with the status and
        // the grid is gone.  Re-run this sentence from its initial state on the multi-launch
        // path (same results within the resident tests' tolerance); the handle stays resident.
        // (inference_truncated's carried state may already be overwritten: that case raises.)
        ++d->res_timeouts;
        if (verbose()) {
            int dbg[3] = {0, 0, 0};
            (void)hipMemcpy(dbg, ra.status, sizeof(dbg), hipMemcpyDeviceToHost);
            fprintf(stderr, "[tts] resident decoder: wait %d timed out at step %d on workgroup %d (L=%d); "
                            "re-running multi-launch\n", dbg[0], dbg[1], dbg[2], c.lens[0]);
        }
        return restart_multilaunch(d, c);
    }
    TTS_CHECK(status == 0, TTS_ERR_HIP,
              status == 100 ? "decoder did not stop within max_steps + 20 (internal error)"
                            : "resident decoder: a hand-off wait timed out (internal error)");
    c.run = c.n_steps[0];
    d->last_resident = 1;
    d->res_place_fails = 0;
    *served = true;
    return TTS_OK;
}

// The step graphs: the first chunk without a host wait, then CHUNK steps per poll of n_active.
tts_status run_multilaunch(tts_decoder* d, RunCtx& c) {
    const int B = c.B;
    hipStream_t s = c.s;
    auto key = std::make_tuple(B, c.Lmax, c.max_steps);
    auto it = d->graphs.find(key);
    if (it == d->graphs.end()) {
        StepGraphs g;
        TTS_TRY(build_step_graphs(g, CHUNK, d->stream,
                             [&](int p) { return enqueue_step(d, B, c.Lmax, c.max_steps, p, d->stream); }));
        it = d->graphs.emplace(key, g).first;
    }
    const StepGraphs& g = it->second;
    if (c.timed) TTS_HIP(hipEventRecord(d->ev_t0, s));
    TTS_TRY(launch_steps(g, CHUNK, c.run, c.first, s));
    for (;;) {
        // n_active as seen by the next step (its parity slot)
        TTS_HIP(hipMemcpyAsync(d->host_flags, d->state + 2 * (c.run & 1), 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        TTS_HIP(spin_sync(s, d->ev_sync));
        if (d->host_flags[1] == 0) break;
        TTS_CHECK(c.run < c.max_steps + 20, TTS_ERR_HIP, "decoder did not stop within max_steps + 20 (internal error)");
        TTS_TRY(launch_steps(g, CHUNK, c.run, CHUNK, s));
    }
    if (c.timed) TTS_HIP(hipEventRecord(d->ev_t1, s));
    TTS_HIP(hipMemcpyAsync(d->host_flags + 4, d->n_steps, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    if (d->io_rb_src) TTS_HIP(hipMemcpyAsync(d->io_rb_dst, d->io_rb_src, sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP(spin_sync(s, d->ev_sync));
    std::copy(d->host_flags + 4, d->host_flags + 4 + B, c.n_steps);
    return TTS_OK;
}

// mel / stop / alignment rows [0, max n_steps) of every sentence to the caller's buffers, zero past
// each sentence's own n_steps.
tts_status copy_out(tts_decoder* d, const RunCtx& c, int steps_cap, float* mel, float* stop, float* align) {
    const int B = c.B, Lmax = c.Lmax;
    hipStream_t s = c.s;
    int nmax = 0;
    for (int b = 0; b < B; ++b) nmax = std::max(nmax, (int)c.n_steps[b]);
    const size_t nm = d->nmel;
    TTS_HIP(hipMemcpy2DAsync(mel, (size_t)steps_cap * nm * 4, d->mel_hist, (size_t)d->hist_cap * nm * 4,
                             (size_t)nmax * nm * 4, B, hipMemcpyDeviceToDevice, s));
    TTS_HIP(hipMemcpy2DAsync(stop, (size_t)steps_cap * 4, d->stop_hist, (size_t)d->hist_cap * 4, (size_t)nmax * 4, B,
                             hipMemcpyDeviceToDevice, s));
    if (align)
        TTS_HIP(hipMemcpy2DAsync(align, (size_t)steps_cap * Lmax * 4, d->align_hist, (size_t)d->hist_cap * Lmax * 4,
                                 (size_t)nmax * Lmax * 4, B, hipMemcpyDeviceToDevice, s));
    // the mel history is written unguarded by done[] (see EPI_MEL_FUSED): zero rows past n_steps
    TTS_HIP(launch_zero_tail(mel, (int64_t)steps_cap * nm, d->n_steps, (int)nm, nmax, B, s));
    // stop and alignment rows are written under done[]: past n_steps the histories still hold the
    // rows of an earlier, longer run in this slot (batch 1 has no such rows: nmax = n_steps[0])
    if (B > 1) {
        TTS_HIP(launch_zero_tail(stop, steps_cap, d->n_steps, 1, nmax, B, s));
        if (align) TTS_HIP(launch_zero_tail(align, (int64_t)steps_cap * Lmax, d->n_steps, Lmax, nmax, B, s));
    }
    return TTS_OK;
}

tts_status decoder_run(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax, int max_steps,
                       int steps_cap, float* mel, float* stop, float* align, int32_t* n_steps, void* stream, bool keep) {
    TTS_CHECK(d && enc && lens && mel && stop && n_steps, TTS_ERR_INVALID, "null argument");
    TTS_CHECK(B >= 1 && B <= d->Bcap, TTS_ERR_INVALID, "batch exceeds decoder capacity");
    TTS_CHECK(Lmax >= 2 && Lmax <= d->Lcap, TTS_ERR_INVALID, "Lmax exceeds decoder capacity");
    TTS_CHECK(max_steps >= 1 && max_steps <= d->cfg.max_steps, TTS_ERR_INVALID, "max_steps exceeds decoder capacity");
    TTS_CHECK(steps_cap >= max_steps + 20, TTS_ERR_INVALID, "steps_cap must be >= max_steps + 20");
    hipStream_t cs = static_cast<hipStream_t>(stream);
    RunCtx c{};
    c.enc = enc; c.lens = lens; c.n_steps = n_steps;
    c.B = B; c.Lmax = Lmax; c.max_steps = max_steps;
    c.s = d->pipeline ? cs : d->stream;
    c.keep = keep;
    // stage timers (tts_decoder_last_timing) outside pipeline mode only: every event marker holds
    // the GPU ~5.8 us between the kernels around it
    c.timed = !d->pipeline;
    TTS_TRY(stage_inputs(d, c, cs));
    d->last_resident = 0;
    if (verbose())
        fprintf(stderr, "[tts] decoder_run B=%d L=%d resident=%d gen=%d keep=%d direct=%d\n", B, lens[0],
                (int)d->resident, d->res_gen, (int)keep, (int)c.direct);
    bool served = false;
    TTS_TRY(run_resident_batch(d, c, &served));
    if (!served) TTS_TRY(run_resident_one(d, c, &served));
    if (!served) TTS_TRY(run_multilaunch(d, c));
    if (!d->keep_hist) TTS_TRY(copy_out(d, c, steps_cap, mel, stop, align));
    if (c.s != cs) {
        TTS_HIP(hipEventRecord(d->ev_out, c.s));
        TTS_HIP(hipStreamWaitEvent(cs, d->ev_out, 0));
    }
    d->last_ms = 0.f;  // (pipeline mode: not timed)
    if (c.timed) {
        // (the resident paths record ev_t1 after their last host sync: it may still be pending)
        TTS_HIP(hipEventSynchronize(d->ev_t1));
        TTS_HIP(hipEventElapsedTime(&d->last_ms, d->ev_t0, d->ev_t1));
    }
    d->last_steps = c.run;
    d->last_B = B;
    d->last_Lmax = Lmax;
    d->last_max_steps = max_steps;
    d->last_first = c.first;
    d->last_init = c.ia;
    d->last_init.keep = 0;
    d->last_steps_done = B == 1 ? (int)n_steps[0] : 0;
    return TTS_OK;
}
}  // namespace

extern "C" {

tts_status tts_decoder_create(const tts_decoder_config* cfg, const tts_tensor* tensors, int n_tensors, void* stream,
                              tts_decoder** out) {
    TTS_CHECK(cfg && out && (tensors || n_tensors == 0), TTS_ERR_INVALID, "null argument");
    TTS_CHECK(cfg->r >= 1 && cfg->r <= 8, TTS_ERR_INVALID, "r must be in [1, 8]");
    TTS_CHECK(cfg->max_batch >= 1 && cfg->max_batch <= 64, TTS_ERR_UNSUPPORTED, "max_batch must be in [1, 64]");
    TTS_CHECK(cfg->max_len >= 2 && cfg->max_len <= (cfg->location_attn ? 512 : 1024), TTS_ERR_UNSUPPORTED,
              "max_len must be in [2, 1024] (512 with location attention)");
    TTS_CHECK(cfg->max_steps >= 1, TTS_ERR_INVALID, "max_steps must be >= 1");
    TTS_CHECK(cfg->attn_norm == 0 || cfg->attn_norm == 1, TTS_ERR_INVALID, "Unknown value for attention norm type");
    TTS_CHECK(!cfg->trans_agent || cfg->forward_attn, TTS_ERR_INVALID, "trans_agent requires forward_attn");
    auto* d = new tts_decoder();
    d->cfg = *cfg;
    d->nmel = 80 * cfg->r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto fail = [&](tts_status code) { tts_decoder_destroy(d); return code; };
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_out, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_t0, hipEventReleaseToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_t1, hipEventReleaseToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_sync, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&d->host_flags), (4 + 64) * sizeof(int), hipHostMallocCoherent) != hipSuccess) {
        set_error("stream/event creation failed");
        return fail(TTS_ERR_HIP);
    }
    // the host polls host_flags[3] for ++rb_seq (from 1): a recycled pinned block could still hold
    // an earlier handle's sequence value, so the words start at zero
    std::memset(d->host_flags, 0, (4 + 64) * sizeof(int));
    const WeightMap wm(tensors, n_tensors);
    SrcWeights w{};
    tts_status st = lookup_weights(d, wm, w);
    if (!st) st = create_weights(d, wm, w, s);
    if (!st) st = create_workspace(d, s);
    if (st) return fail(st);
    *out = d;
    return TTS_OK;
}

void tts_decoder_destroy(tts_decoder* d) {
    if (!d) return;
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    for (auto& kv : d->graphs) destroy_step_graphs(kv.second);
    d->dev.free_all();
    if (d->host_flags) (void)hipHostFree(d->host_flags);
    for (hipEvent_t e : {d->ev_in, d->ev_out, d->ev_t0, d->ev_t1, d->ev_sync})
        if (e) (void)hipEventDestroy(e);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

tts_status tts_decoder_run(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax, int max_steps,
                           int steps_cap, float* mel, float* stop, float* align, int32_t* n_steps, void* stream) {
    return decoder_run(d, enc, lens, B, Lmax, max_steps, steps_cap, mel, stop, align, n_steps, stream, false);
}

tts_status tts_decoder_run_teacher(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax,
                                   const float* memories, int64_t mem_ldb, int steps, float* mel, float* stop,
                                   float* align, void* stream) {
    TTS_CHECK(d && enc && lens && memories && mel && stop, TTS_ERR_INVALID, "null argument");
    TTS_CHECK(B >= 1 && B <= d->Bcap, TTS_ERR_INVALID, "batch exceeds decoder capacity");
    TTS_CHECK(Lmax >= 2 && Lmax <= d->Lcap, TTS_ERR_INVALID, "Lmax exceeds decoder capacity");
    TTS_CHECK(steps >= 1 && steps <= d->hist_cap, TTS_ERR_INVALID, "teacher steps exceed the decoder's history capacity");
    TTS_CHECK(mem_ldb >= (int64_t)(steps - 1) * d->nmel, TTS_ERR_INVALID, "teacher memory rows too short");
    for (int b = 0; b < B; ++b)
        TTS_CHECK(lens[b] >= 2 && lens[b] <= Lmax, TTS_ERR_INVALID, "encoder length out of range [2, Lmax]");
    hipStream_t cs = static_cast<hipStream_t>(stream);
    hipStream_t s = d->stream;
    TTS_HIP(hipEventRecord(d->ev_in, cs));
    TTS_HIP(hipStreamWaitEvent(s, d->ev_in, 0));
    TTS_HIP(hipMemcpy2DAsync(d->enc, (size_t)d->Lcap * ENC * 4, enc, (size_t)Lmax * ENC * 4, (size_t)Lmax * ENC * 4, B,
                             hipMemcpyDeviceToDevice, s));
    TTS_HIP(hipMemcpyAsync(d->lens, lens, sizeof(int) * B, hipMemcpyHostToDevice, s));
    TTS_HIP(launch_project_inputs(d->enc, d->W_in, B, Lmax, d->Lcap, d->Pt, s));
    TTS_HIP(launch_decoder_init(make_init_args(d, B, d->lens), s));
    if (frag_on(d, B)) { tts_status fs = enqueue_frag_sync(d, B, s); if (fs) return fs; }
    // step t: memory = go frame (t = 0) or teacher row t-1 -> prenet layer 1 (reference weights, no
    // fold) -> the inference step with the stop rule off (its fused launch's prenet-1 output is
    // overwritten by the next step's teacher frame)
    for (int t = 0; t < steps; ++t) {
        const int p = t & 1;
        TTS_HIP(launch_teacher_memory(memories, mem_ldb, d->nmel, d->state + 2 * p, d->mem, B, s));
        tts_status st = enqueue_prenet_go(d, B, s, d->state + 2 * p);
        if (!st) st = enqueue_step(d, B, Lmax, steps, p, s, nullptr, 2);
        if (st) return st;
    }
    const size_t nm = d->nmel;
    TTS_HIP(hipMemcpy2DAsync(mel, (size_t)steps * nm * 4, d->mel_hist, (size_t)d->hist_cap * nm * 4, (size_t)steps * nm * 4,
                             B, hipMemcpyDeviceToDevice, s));
    TTS_HIP(hipMemcpy2DAsync(stop, (size_t)steps * 4, d->stop_hist, (size_t)d->hist_cap * 4, (size_t)steps * 4, B,
                             hipMemcpyDeviceToDevice, s));
    if (align)
        TTS_HIP(hipMemcpy2DAsync(align, (size_t)steps * Lmax * 4, d->align_hist, (size_t)d->hist_cap * Lmax * 4,
                                 (size_t)steps * Lmax * 4, B, hipMemcpyDeviceToDevice, s));
    TTS_HIP(hipEventRecord(d->ev_out, s));
    TTS_HIP(hipStreamWaitEvent(cs, d->ev_out, 0));
    d->last_resident = 0;
    d->last_steps_done = 0;  // a later run_continue must start from a regular run
    return TTS_OK;
}

tts_status tts_decoder_run_continue(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax,
                                    int max_steps, int steps_cap, float* mel, float* stop, float* align,
                                    int32_t* n_steps, void* stream) {
    TTS_CHECK(d && B == 1, TTS_ERR_UNSUPPORTED, "continuous (truncated) decoding is batch-1, as the reference's");
    TTS_CHECK(d->last_B == 1 && d->last_steps_done > 0, TTS_ERR_INVALID,
              "tts_decoder_run_continue needs a previous batch-1 tts_decoder_run / _continue");
    return decoder_run(d, enc, lens, B, Lmax, max_steps, steps_cap, mel, stop, align, n_steps, stream, true);
}

}  // extern "C"

namespace {
// Measurement only: re-run the last batch-1 resident sentence with timers (marks: per-phase tick
// sums of CU 0 and the logging attention CU; always: the per-CU event trace, kept in d->res_trace).
tts_status res_rerun(tts_decoder* d, bool marks, long long* h) {
    TTS_CHECK(d->last_resident == 1 && d->last_steps > 0, TTS_ERR_INVALID,
              "the resident decoder profile needs a previous resident tts_decoder_run");
    TTS_HIP(hipDeviceSynchronize());  // measurement only: nothing else (a pipeline GL) on the device
    hipStream_t s = d->stream;
    long long* prof = nullptr;
    TTS_HIP(hipMalloc(&prof, sizeof(long long) * RES_PROF_LL));
    TTS_HIP(hipMemsetAsync(prof, 0, sizeof(long long) * RES_PROF_LL, s));
    TTS_HIP(launch_decoder_init(d->last_init, s));
    tts_status st = enqueue_prenet_go(d, 1, s);
    ResArgs ra = d->last_ra;
    ra.prof = prof;
    ra.prof_marks = marks ? 1 : 0;
    if (!st) {
        TTS_HIP(hipMemsetAsync(d->gran, 0, sizeof(unsigned long long) * (2 * GR_TOTAL + 2), s));
        bool launched = false;
        TTS_HIP(launch_resident(ra, s, &launched));
        if (!launched) {
            (void)hipStreamSynchronize(s);
            (void)hipFree(prof);
            TTS_CHECK(false, TTS_ERR_UNSUPPORTED, "resident decoder cannot be co-resident on this device now");
        }
    }
    TTS_HIP(hipMemcpyAsync(h, prof, sizeof(long long) * 2 * RES_PHASES, hipMemcpyDeviceToHost, s));
    d->res_trace.resize(RES_PROF_LL - 2 * RES_PHASES);
    TTS_HIP(hipMemcpyAsync(d->res_trace.data(), prof + 2 * RES_PHASES, sizeof(long long) * d->res_trace.size(),
                           hipMemcpyDeviceToHost, s));
    TTS_HIP(hipMemcpyAsync(d->host_flags, ra.status, sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipStreamSynchronize(s));
    (void)hipFree(prof);
    if (st) return st;
    TTS_CHECK(d->host_flags[0] == 0, TTS_ERR_HIP, "resident decoder: a hand-off wait timed out (internal error)");
    return TTS_OK;
}
}  // namespace

extern "C" {

tts_status tts_decoder_last_timing(tts_decoder* d, float* loop_ms, int* steps_run) {
    TTS_CHECK(d && loop_ms && steps_run, TTS_ERR_INVALID, "null argument");
    *loop_ms = d->last_ms;
    *steps_run = d->last_steps;
    return TTS_OK;
}

tts_status tts_decoder_resident_limits(tts_decoder* d, int* max_batch, int* max_len) {
    TTS_CHECK(d && max_batch && max_len, TTS_ERR_INVALID, "null argument");
    *max_batch = d->resident ? (d->rbatch ? std::max(1, std::min(d->Bcap, rb_max_batch())) : 1) : 0;
    *max_len = d->resident ? RES_LMAX : 0;
    return TTS_OK;
}

tts_status tts_decoder_last_path(tts_decoder* d, int* resident) {
    TTS_CHECK(d && resident, TTS_ERR_INVALID, "null argument");
    *resident = d->last_resident;
    return TTS_OK;
}

tts_status tts_decoder_resident_phases(tts_decoder* d, float* us, int n) {
    TTS_CHECK(d && us && n >= 2 * RES_PHASES, TTS_ERR_INVALID, "bad arguments");
    long long h[2 * RES_PHASES];
    if (tts_status st = res_rerun(d, true, h)) return st;
    int dev = 0, rate_khz = 1;
    TTS_HIP(hipGetDevice(&dev));
    TTS_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev));
    for (int i = 0; i < 2 * RES_PHASES; ++i) us[i] = (float)(1e3 * (double)h[i] / rate_khz / d->last_steps);
    return TTS_OK;
}

tts_status tts_decoder_resident_trace(tts_decoder* d, long long* ticks, int64_t n) {
    TTS_CHECK(d && ticks && n >= (int64_t)(RES_PROF_LL - 2 * RES_PHASES), TTS_ERR_INVALID, "bad arguments");
    long long h[2 * RES_PHASES];
    if (tts_status st = res_rerun(d, false, h)) return st;  // no phase marks: only the event stamps
    std::copy(d->res_trace.begin(), d->res_trace.end(), ticks);
    return TTS_OK;
}

tts_status tts_decoder_profile(tts_decoder* d, int reps, float* kernel_ms, int n_kernels) {
    TTS_CHECK(d && kernel_ms && n_kernels >= TTS_DECODER_STEP_KERNELS, TTS_ERR_INVALID, "bad profile arguments");
    TTS_CHECK(d->last_B > 0, TTS_ERR_INVALID, "tts_decoder_profile needs a previous tts_decoder_run");
    // every sentence stays active for the first `last_first` steps: time only those
    reps = std::max(1, std::min(reps, d->last_first - 1));
    const int K = TTS_DECODER_STEP_KERNELS;
    hipEvent_t ev[K + 1];
    for (int i = 0; i <= K; ++i) TTS_HIP(hipEventCreate(&ev[i]));
    TTS_HIP(hipDeviceSynchronize());  // measurement only: nothing else (a pipeline GL) on the device
    hipStream_t s = d->stream;
    InitArgs init = d->last_init;
    if (d->last_enc_direct) {
        // the last run read its encoder output and length in place: stage copies for the step
        // graphs.  The length is the run's own (host record: the device word it read may hold a later
        // sentence's by now, possibly longer than this shape); the encoder rows are read from the
        // caller's buffer as it is now (the caller keeps it alive; the step timings do not depend on
        // its contents)
        const int len = d->last_len_direct;
        TTS_HIP(hipMemcpyAsync(d->enc, d->last_enc_direct, (size_t)d->last_Lmax * ENC * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
        TTS_HIP(hipMemcpyAsync(d->lens, &len, sizeof(int), hipMemcpyHostToDevice, s));
        TTS_HIP(hipStreamSynchronize(s));  // `len` is a stack copy
        init.lens = d->lens;
    }
    TTS_HIP(launch_decoder_init(init, s));
    tts_status st = enqueue_prenet_go(d, d->last_B, s);
    std::vector<double> acc(K, 0.0);
    for (int r = 0; r < reps && st == TTS_OK; ++r) {
        st = enqueue_step(d, d->last_B, d->last_Lmax, d->last_max_steps, r & 1, s, ev);
        if (st) break;
        TTS_HIP(hipEventSynchronize(ev[K]));
        for (int i = 0; i < K; ++i) {
            float ms = 0.f;
            TTS_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            acc[i] += ms;
        }
    }
    for (int i = 0; i <= K; ++i) (void)hipEventDestroy(ev[i]);
    if (st) return st;
    for (int i = 0; i < K; ++i) kernel_ms[i] = (float)(acc[i] / reps);
    return TTS_OK;
}

}  // extern "C"

namespace tts {
void decoder_set_pipeline(tts_decoder* d, bool on) {
    d->pipeline = on;
    d->keep_hist = on;
    if (!on) {
        d->post_hook = nullptr;
        decoder_set_pipeline_io(d, nullptr, nullptr, nullptr, nullptr, 0);
    }
}
void decoder_set_pipeline_io(tts_decoder* d, const int* lens_dev, const int* rb_src, int* rb_dst, int* clamp_dst,
                             int clamp_max) {
    d->io_lens = lens_dev;
    d->io_rb_src = rb_src;
    d->io_rb_dst = rb_dst;
    d->io_clamp = clamp_dst;
    d->io_clamp_max = clamp_max;
}
void decoder_set_post_hook(tts_decoder* d, void (*fn)(void*, hipStream_t), void* ctx) {
    d->post_hook = fn;
    d->post_ctx = ctx;
    d->hook_ran = false;
}
bool decoder_hook_ran(tts_decoder* d) { return d->hook_ran && d->last_resident == 1; }
void decoder_histories(tts_decoder* d, const float** mel, int64_t* sentence_floats, const int** n_steps) {
    *mel = d->mel_hist;
    *sentence_floats = (int64_t)d->hist_cap * d->nmel;
    *n_steps = d->n_steps;
}
}  // namespace tts
