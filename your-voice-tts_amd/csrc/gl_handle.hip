// The Griffin-Lim / AudioProcessor handle's life: the constant tables of its geometry, its stream
// and events, and what the last run left for the host to read.
#include <cmath>
#include <vector>

#include "gl_handle.h"

using namespace tts;

namespace tts {
void gl_set_pipeline(tts_gl* g, bool on) { g->pipeline = on; }
}  // namespace tts

extern "C" {

void tts_gl_destroy(tts_gl* g) {
    if (!g) return;
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->ev_done) (void)hipEventSynchronize(g->ev_done);  // a pipeline run on another stream
    if (g->mt_stream) (void)hipEventSynchronize(g->ev_mt);  // the last numpy-stream phase draw
    mt_work_free(&g->mt_work);
    for (auto& kv : g->graphs) (void)hipGraphExecDestroy(kv.second);
    for (void* p : {(void*)g->win, (void*)g->win2, (void*)g->pinv, (void*)g->tw, (void*)g->S.p, (void*)g->frames.p,
                    (void*)g->y.p, (void*)g->F.p, (void*)g->basis, (void*)g->band, (void*)g->NS.p, (void*)g->flags.p,
                    (void*)g->pstatus, (void*)g->pgr.p, (void*)g->wt, (void*)g->winc, (void*)g->wssp,
                    (void*)g->mt_state, (void*)g->mt_phase.p, (void*)g->mt_F.p, (void*)g->pcm_peak,
                    (void*)g->pcm_start.p, (void*)g->sil.p, (void*)g->seg.p, (void*)g->rs_win.p,
                    (void*)g->rs_sent.p})
        if (p) (void)hipFree(p);
    for (auto& kv : g->rs_reg)
        if (kv.second.dev.p) (void)hipFree(kv.second.dev.p);
    if (g->host_status) (void)hipHostFree(g->host_status);
    for (hipEvent_t e : {g->ev_in, g->ev_out, g->ev_t0, g->ev_t1, g->ev_done, g->ev_mt})
        if (e) (void)hipEventDestroy(e);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

tts_status tts_gl_create(const tts_audio_config* cfg, const double* inv_mel_basis, void* stream, tts_gl** out) {
    TTS_CHECK(cfg && out, TTS_ERR_INVALID, "null argument");
    TTS_CHECK(cfg->n_fft == NFFT, TTS_ERR_UNSUPPORTED, "n_fft must be 2048 (num_freq 1025)");
    TTS_CHECK(cfg->win_length >= 2 && cfg->win_length <= NFFT, TTS_ERR_INVALID, "win_length must be in [2, n_fft]");
    TTS_CHECK(cfg->hop_length >= 1 && cfg->hop_length <= cfg->win_length, TTS_ERR_UNSUPPORTED,
              "hop_length must be in [1, win_length]");
    TTS_CHECK(cfg->num_mels >= 1 && cfg->num_mels <= 80, TTS_ERR_UNSUPPORTED, "num_mels must be <= 80");
    auto* g = new tts_gl();
    g->cfg = *cfg;
    g->g.hop = cfg->hop_length;
    g->g.win = cfg->win_length;
    g->g.woff = (NFFT - cfg->win_length) / 2;  // librosa util.pad_center
    g->g.fb = g->g.woff & ~1;
    g->g.winp = (cfg->win_length + (g->g.woff - g->g.fb) + 3) / 4 * 4;
    (void)stream;
    std::vector<double> win(NFFT, 0.0), win2(NFFT, 0.0);
    for (int n = 0; n < cfg->win_length; ++n) {
        const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / cfg->win_length);  // periodic Hann
        win[g->g.woff + n] = w;
        win2[g->g.woff + n] = w * w;
    }
    std::vector<double2> tw(NFFT);
    for (int m = 0; m < NFFT; ++m) tw[m] = double2{std::cos(2.0 * M_PI * m / NFFT), -std::sin(2.0 * M_PI * m / NFFT)};
    // a failed HIP call destroys the half-built handle
    auto ok = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return TTS_OK;
        tts_status st = hip_fail(e, what, __FILE__, __LINE__);
        tts_gl_destroy(g);
        return st;
    };
    // a device copy of a host vector
    auto upload = [&](auto** dst, const auto& v) {
        const size_t bytes = v.size() * sizeof(v[0]);
        if (tts_status st = ok(hipMalloc(dst, bytes), "hipMalloc")) return st;
        return ok(hipMemcpy(*dst, v.data(), bytes, hipMemcpyHostToDevice), "copy");
    };
    TTS_TRY(ok(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking), "stream"));
    for (hipEvent_t* ev : {&g->ev_in, &g->ev_out, &g->ev_done, &g->ev_mt})
        TTS_TRY(ok(hipEventCreateWithFlags(ev, hipEventDisableTiming), "event"));
    for (hipEvent_t* ev : {&g->ev_t0, &g->ev_t1})
        TTS_TRY(ok(hipEventCreateWithFlags(ev, hipEventReleaseToDevice), "event"));
    TTS_TRY(upload(&g->win, win));
    TTS_TRY(upload(&g->win2, win2));
    TTS_TRY(upload(&g->tw, tw));
    {
        // wt[q2][p1] = W64^(p1 q2): the pass-2 twiddles of gl_iter_wave_kernel
        std::vector<double2> wt(64);
        for (int q2 = 0; q2 < 16; ++q2)
            for (int p1 = 0; p1 < 4; ++p1) {
                const double a2 = 2.0 * M_PI * (double)(p1 * q2) / 64.0;
                wt[q2 * 4 + p1] = double2{std::cos(a2), -std::sin(a2)};
            }
        TTS_TRY(upload(&g->wt, wt));
        // window cosine seeds (c_0, c_1), c_r = cos(2 pi (s + 128 r - woff) / win), at the first sample
        // of each lane: input order (s = 2 L + e), output order (s = 2 (16 (L & 3) + (L >> 2)) + e)
        std::vector<double2> wc(4 * 64);
        for (int L = 0; L < 64; ++L)
            for (int e = 0; e < 2; ++e) {
                const int si = 2 * L + e, so = 2 * (16 * (L & 3) + (L >> 2)) + e;
                const double ai = 2.0 * M_PI * (double)(si - g->g.woff) / cfg->win_length;
                const double ao = 2.0 * M_PI * (double)(so - g->g.woff) / cfg->win_length;
                const double ar = 2.0 * M_PI * 128.0 / cfg->win_length;
                wc[e * 64 + L] = double2{std::cos(ai), std::cos(ai + ar)};
                wc[(2 + e) * 64 + L] = double2{std::cos(ao), std::cos(ao + ar)};
            }
        g->wrot = 2.0 * std::cos(2.0 * M_PI * 128.0 / cfg->win_length);
        TTS_TRY(upload(&g->winc, wc));
        g->wave = !env_is("TTS_GL_WAVE", '0');
        // window sum-square of a sample q (u = q - woff) with every contributor present: frames
        // i = ceil((u - win + 1) / hop) .. floor(u / hop) in index order, float32 additions of the
        // float64 win^2 as ola_sample makes them; depends on u mod hop only
        const int hop = cfg->hop_length, wl = cfg->win_length;
        std::vector<float> wp(hop);
        for (int r = 0; r < hop; ++r) {
            const int u = r + hop * (wl / hop + 1);
            const int ilo = (u - wl + 1 + hop - 1) / hop, ihi = u / hop;
            float w = 0.f;
            for (int i = ilo; i <= ihi; ++i) w = (float)((double)w + win2[g->g.woff + u - i * hop]);
            wp[r] = w;
        }
        TTS_TRY(upload(&g->wssp, wp));
    }
    if (inv_mel_basis) {
        std::vector<double> pt((size_t)NB * cfg->num_mels);
        for (int k = 0; k < NB; ++k)
            for (int m = 0; m < cfg->num_mels; ++m) pt[(size_t)m * NB + k] = inv_mel_basis[(size_t)k * cfg->num_mels + m];
        TTS_TRY(upload(&g->pinv, pt));
    }
    // persistent GL loop: status word, timeout (50 ms per wait); needs >= 256 compute units
    {
        int dev = 0, ncu = 0, rate_khz = 0;
        TTS_TRY(ok(hipMalloc(&g->pstatus, 16), "hipMalloc"));
        // (an empty speculative run leaves the word as it is: it must start out clean)
        TTS_TRY(ok(hipMemset(g->pstatus, 0, 16), "hipMemset"));
        TTS_TRY(ok(hipHostMalloc(reinterpret_cast<void**>(&g->host_status), 2 * sizeof(int), hipHostMallocCoherent),
                   "hipHostMalloc"));
        // host_status[1] is polled for ++seq (from 1): a recycled pinned block may hold a stale match
        g->host_status[0] = 0;
        g->host_status[1] = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu >= 256 &&
            hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && rate_khz > 0)
            g->tmo = (long long)rate_khz * 50;
        // tests only: a tiny per-wait budget forces the timeout path (status, NaN-poisoned signal)
        const char* tk = getenv("TTS_GL_WAIT_TICKS");
        if (tk && tk[0] && g->tmo > 0) g->tmo = std::max(1LL, atoll(tk));
    }
    *out = g;
    return TTS_OK;
}

tts_status tts_gl_last_path(tts_gl* g, int* path) {
    TTS_CHECK(g && path, TTS_ERR_INVALID, "null argument");
    *path = g->last_path;
    return TTS_OK;
}

tts_status tts_gl_last_timing(tts_gl* g, float* loop_ms, int* launches) {
    TTS_CHECK(g && loop_ms && launches, TTS_ERR_INVALID, "null argument");
    TTS_TRY(gl_collect(g));
    *loop_ms = g->last_ms;
    *launches = g->last_launches;
    return TTS_OK;
}

}  // extern "C"
