// librosa.load(filename, sr=sr)'s resampler (utils/audio.py:239) on ragged batches in HBM: librosa 0.6.2
// resample(fix=True) = resampy 0.2.x resample_f with the caller's half window (kaiser_best: 32 769 values,
// 512 per zero crossing), then fix_length.  Per sentence ratio = target_sr / orig_sr, n_res = int(N ratio)
// outputs, scale = min(1, ratio), step = int(scale num_table), win[o] = half_win[o] ratio when ratio < 1.
// Output t reads the time register tr[t] (n = int(tr[t]), frac = scale (tr[t] - n)) and walks two wings:
//   left : idx = frac num_table, off = int(idx), eta = idx - off,
//          i < min(n + 1, (nwin - off) / step):       y += (win[off + i step] + eta delta[off + i step]) x[n - i]
//   right: the same from frac' = scale - frac, k < min(N - n - 1, (nwin - off) / step), on x[n + k + 1]
// with delta[o] = win[o + 1] - win[o] (0 at the last entry).  The accumulator y is FLOAT32 (resampy's output
// takes x's dtype): every tap is one fp64 multiply, one fp64 add and one rounding to float32, and the taps
// of an output are one dependent chain in resampy's order.  Nothing is fused (-ffp-contract=off) and nothing
// is reordered, so the result is the restatement's bit for bit.  Parallelism is over outputs only.
//
// The time register is resampy's serial sum tr[t] = fl(tr[t - 1] + inc), inc = 1 / ratio: t inc is another
// number (int(tr[t]) differs at 9 of 1378 outputs for 3000 samples 48 000 -> 22 050).  It is summed on the
// host, once per (orig_sr, target_sr), cached on the handle, grown on demand and mirrored on the device.
//
// One launch per call.  The grid is the number of chunks of RS chunk outputs over all sentences (a workgroup
// finds its sentence by bisection over the first-chunk table, as losses.hip does); every thread owns one
// output of its chunk.  A chunk's inputs x[n_first - taps + 1 .. n_last + taps] are staged once in LDS as the
// float32 values librosa hands resampy (neighbouring outputs share all but `inc` of their 2 taps inputs).
// The table stays in its base layout: off <= step for every output, so tap i of every output falls into the
// one window half_win[i step .. (i + 1) step + 1] (1.9 KB at 48 -> 22.05 kHz, 4 KB when upsampling), the
// same window for every wave of the device at that tap, shared through L2.  Consecutive outputs scatter
// over that window, so outputs go to lanes in the order of their offsets (a rank within the chunk): a
// wave's 64 lanes then read a quarter of the window, 4 to 9 cache lines per tap instead of 16 to 33
// (measured: 1.94 -> 1.07 ms for 32 x 10 s at 48 -> 22.05 kHz; DESIGN "Resampling").  win and delta are formed from
// the base table on the fly with the operations that build the per-ratio tables (half_win[o] ratio,
// half_win[o + 1] ratio, subtract), so no per-ratio table exists; the device copy carries one extra entry
// equal to its last, which makes delta[last] the 0 resampy defines.
// No sample at or beyond N[b] is read; dst is zero from n_res to dst_pitch (fix_length's padding and the
// batch's); a sentence whose rate is already the target passes through (rounded to float32 like the rest).
#include <algorithm>
#include <cmath>

#include "gl_handle.h"

namespace tts {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_FLOATS = 16384;  // 64 KB: the staged inputs of a chunk

struct RsArgs {
    const double* src;
    int64_t src_pitch;
    double* dst;
    int64_t dst_pitch;
    const double* hw;  // [nwin + 1] half window, the last entry repeated
    int nwin, table;
    const RsSent* sent;  // [B]
    int B;
    int chunk;       // outputs per workgroup, <= RS_THREADS
    int lds_floats;  // staged inputs a workgroup may hold
};

typedef double double2u __attribute__((ext_vector_type(2), aligned(8)));

// one wing of one output: `taps` dependent steps over the table entries h[0], h[step], ... and the inputs
// x[0], x[dir], x[2 dir], ...
__device__ __forceinline__ float wing(float y, const double* __restrict__ h, int step, double mult, double eta,
                                      const float* x, int dir, int taps) {
#pragma unroll 4
    for (int i = 0; i < taps; ++i) {
        const double2u hh = *reinterpret_cast<const double2u*>(h);  // one 16-byte load, 8-byte aligned
        const double w0 = hh[0] * mult, w1 = hh[1] * mult;
        const double w = w0 + eta * (w1 - w0);
        y = (float)((double)y + w * (double)x[0]);
        h += step;
        x += dir;
    }
    return y;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsArgs a) {
    extern __shared__ float xs[];
    __shared__ int keys[RS_THREADS];
    __shared__ unsigned char perm[RS_THREADS];
    static_assert(RS_THREADS <= 256, "perm holds a thread index in a byte");
    const int blk = blockIdx.x, tid = threadIdx.x;
    int lo = 0, hi = a.B;  // first[lo] <= blk < first[hi]: the last sentence that starts at or before blk
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.sent[mid].first <= blk) lo = mid;
        else hi = mid;
    }
    const int b = lo;
    const RsSent s = a.sent[b];
    const int t0 = (blk - s.first) * a.chunk;
    const int cnt = min(a.chunk, s.n_res - t0);  // >= 1: the host counted this chunk
    const double* x = a.src + (int64_t)b * a.src_pitch;
    double* y = a.dst + (int64_t)b * a.dst_pitch;
    if (s.tr == nullptr) {  // (block-uniform) already at the target rate
        if (tid < cnt) y[t0 + tid] = (double)(float)x[t0 + tid];
    } else {
        const int taps_max = a.nwin / s.step;
        const int n_first = (int)s.tr[t0], n_last = (int)s.tr[t0 + cnt - 1];
        const int w_lo = max(0, n_first - taps_max + 1);
        int w_hi = min(s.N, n_last + 1 + taps_max);
        w_hi = min(w_hi, w_lo + a.lds_floats);  // (never binds: the host sized chunk and lds_floats for it)
        for (int j = tid; j < w_hi - w_lo; j += RS_THREADS) xs[j] = (float)x[w_lo + j];
        // Outputs to lanes by table offset: thread tid ranks its own output's left-wing offset among the
        // chunk's (keys are unique, so the ranks are a permutation) and takes the output of its rank.  A
        // wave then holds 64 neighbouring offsets, a quarter of the window, in both wings (the right
        // wing's offset falls as the left one rises).  Which lane computes an output changes no bit of it.
        int key = (0x7fffff << 8) | tid;  // (no output: behind every output)
        if (tid < cnt) {
            const double tr = s.tr[t0 + tid];
            const double idx = s.scale * (tr - (double)(int)tr) * (double)a.table;
            key = (min((int)idx, 0x7ffffe) << 8) | tid;
        }
        keys[tid] = key;
        __syncthreads();
        int rank = 0;
        for (int j = 0; j < RS_THREADS; ++j) rank += keys[j] < key;
        perm[rank] = (unsigned char)tid;
        __syncthreads();
        const int me = perm[tid];
        if (me < cnt) {
            const double tr = s.tr[t0 + me];
            const int n = (int)tr;
            double frac = s.scale * (tr - (double)n);
            double idx = frac * (double)a.table;
            int off = (int)idx;
            float acc = wing(0.f, a.hw + off, s.step, s.mult, idx - (double)off, xs + (n - w_lo), -1,
                             min(n + 1, (a.nwin - off) / s.step));
            frac = s.scale - frac;
            idx = frac * (double)a.table;
            off = (int)idx;
            acc = wing(acc, a.hw + off, s.step, s.mult, idx - (double)off, xs + (n + 1 - w_lo), 1,
                       min(s.N - n - 1, (a.nwin - off) / s.step));
            y[t0 + me] = (double)acc;
        }
    }
    if (t0 + cnt == s.n_res)  // the sentence's last chunk: fix_length's zero and the batch's padding
        for (int64_t j = (int64_t)s.n_res + tid; j < a.dst_pitch; j += RS_THREADS) y[j] = 0.0;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_gl_set_resample_filter(tts_gl* g, const double* half_win, int n_win, int num_table) {
    TTS_CHECK(g && half_win, TTS_ERR_INVALID, "set_resample_filter: null argument");
    TTS_CHECK(n_win >= 1 && num_table >= 1, TTS_ERR_INVALID,
              "set_resample_filter: n_win and num_table must be positive");
    // (tts_gl_resample waits for its stream before it returns: the previous table is idle)
    TTS_TRY(g->rs_win.reserve((size_t)n_win + 1));
    std::vector<double> h(half_win, half_win + n_win);
    h.push_back(h.back());  // delta[last] = 0
    TTS_HIP(hipMemcpy(g->rs_win.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    g->rs_nwin = n_win;
    g->rs_table = num_table;
    return TTS_OK;
}

tts_status tts_gl_resample(tts_gl* g, const double* src, int64_t src_pitch, const int32_t* N,
                           const int32_t* orig_sr, int target_sr, int B, double* dst, int64_t dst_pitch,
                           int32_t* n_out, void* stream) {
    TTS_CHECK(g && src && N && orig_sr && dst && n_out, TTS_ERR_INVALID, "resample: null argument");
    TTS_CHECK(B >= 1, TTS_ERR_INVALID, "resample: B must be positive");
    TTS_CHECK(target_sr >= 1, TTS_ERR_INVALID, "resample: target_sr must be positive");
    TTS_CHECK(dst_pitch <= INT32_MAX, TTS_ERR_INVALID, "resample: dst_pitch out of range");
    TTS_CHECK(g->rs_nwin >= 1, TTS_ERR_INVALID, "resample: no filter set (tts_gl_set_resample_filter)");
    const int nwin = g->rs_nwin, table = g->rs_table;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<RsSent>& sent = g->rs_sent_h;
    sent.assign(B, RsSent{});
    int chunk = RS_THREADS;
    // the arithmetic of resampy.resample and librosa's fix_length, in Python's order
    for (int b = 0; b < B; ++b) {
        const std::string who = "resample: sentence " + std::to_string(b);
        TTS_CHECK(orig_sr[b] >= 1, TTS_ERR_INVALID, who + " has a non-positive orig_sr");
        TTS_CHECK(N[b] >= 1 && N[b] <= src_pitch, TTS_ERR_INVALID, who + " has N[b] out of range [1, src_pitch]");
        const double ratio = (double)target_sr / (double)orig_sr[b];
        const double len = (double)N[b] * ratio;
        TTS_CHECK(len >= 1.0, TTS_ERR_INVALID,
                  who + " is too short to resample (n_res = int(N * target_sr / orig_sr) < 1)");
        TTS_CHECK(std::ceil(len) <= (double)dst_pitch, TTS_ERR_INVALID, who + " has n_fix > dst_pitch");
        RsSent& d = sent[b];
        d.N = N[b];
        d.n_res = (int)len;
        n_out[b] = (int)std::ceil(len);
        if (orig_sr[b] == target_sr) continue;  // pass-through: tr stays null
        d.scale = std::min(1.0, ratio);
        d.mult = ratio < 1.0 ? ratio : 1.0;
        d.step = (int)(d.scale * (double)table);
        TTS_CHECK(d.step >= 1, TTS_ERR_INVALID,
                  who + " has step = int(min(1, ratio) * num_table) < 1: the filter table is too coarse for its ratio");
        const double inc = 1.0 / ratio;
        RsRegister& r = g->rs_reg[{orig_sr[b], target_sr}];
        if (r.host.empty()) r.host.push_back(0.0);
        while (r.host.size() < (size_t)d.n_res) r.host.push_back(r.host.back() + inc);  // serial: the contract
        TTS_CHECK((int)r.host[d.n_res - 1] < d.N, TTS_ERR_INVALID,
                  who + " has a time register that leaves the signal (int(tr[n_res - 1]) >= N)");
        // the inputs a chunk of outputs touches: (chunk - 1) inc + 1 between its first and last centre, a wing
        // of at most nwin / step on either side
        const int64_t taps = nwin / d.step;
        while (chunk > 1 && (int64_t)((chunk - 1) * inc) + 3 + 2 * taps > RS_LDS_FLOATS) chunk >>= 1;
        TTS_CHECK((int64_t)((chunk - 1) * inc) + 3 + 2 * taps <= RS_LDS_FLOATS, TTS_ERR_INVALID,
                  who + " has filter wings of " + std::to_string(taps) + " taps: more than the staging window holds");
    }
    int64_t chunks = 0;
    int lds_floats = 1;
    for (int b = 0; b < B; ++b) {
        RsSent& d = sent[b];
        d.first = (int)chunks;
        chunks += (d.n_res + chunk - 1) / chunk;
        TTS_CHECK(chunks <= INT32_MAX, TTS_ERR_INVALID, "resample: more than 2^31 - 1 chunks of work");
        if (orig_sr[b] == target_sr) continue;
        RsRegister& r = g->rs_reg[{orig_sr[b], target_sr}];
        if (r.uploaded < (size_t)d.n_res) {  // (idle: every call waits for its stream before it returns)
            TTS_TRY(r.dev.reserve(r.host.size()));
            TTS_HIP(hipMemcpyAsync(r.dev.p, r.host.data(), r.host.size() * sizeof(double), hipMemcpyHostToDevice, s));
            r.uploaded = r.host.size();
        }
        const double inc = 1.0 / ((double)target_sr / (double)orig_sr[b]);
        lds_floats = std::max<int64_t>(lds_floats, (int64_t)((chunk - 1) * inc) + 3 + 2 * (nwin / d.step));
    }
    for (int b = 0; b < B; ++b)  // (after the last reserve: a register's block may have moved)
        if (orig_sr[b] != target_sr) sent[b].tr = g->rs_reg[{orig_sr[b], target_sr}].dev.p;
    TTS_TRY(g->rs_sent.reserve(B));
    TTS_HIP(hipMemcpyAsync(g->rs_sent.p, sent.data(), B * sizeof(RsSent), hipMemcpyHostToDevice, s));
    RsArgs a{src, src_pitch, dst, dst_pitch, g->rs_win.p, nwin, table, g->rs_sent.p, B, chunk, lds_floats};
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)chunks), dim3(RS_THREADS), lds_floats * sizeof(float), s, a);
    TTS_HIP(hipGetLastError());
    TTS_HIP(hipStreamSynchronize(s));
    return TTS_OK;
}

}  // extern "C"
