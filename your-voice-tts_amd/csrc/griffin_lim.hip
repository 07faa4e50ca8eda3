// Batched Griffin-Lim vocoder (AudioProcessor.inv_mel_spectrogram / inv_spectrogram,
// utils/audio.py:154-201, librosa 0.6.2 stft/istft semantics) for gfx950.
//
// Precision follows the reference exactly where it is observable: the magnitude |S|^power and
// every FFT are float64 (scipy.fftpack on float64 frames), the STFT matrix is rounded to
// complex64 before the phase is taken (librosa stft's dtype), and the overlap-added signal y is
// float32 (librosa istft's dtype), accumulated frame by frame in float32 as librosa does.  GL
// amplifies rounding ~100x over 60 iterations, so this is what keeps the waveform within 1e-4.
//
// HBM layout (per call):
//   S      [B][Fmax][1025] f32    |S|^power, frame-major (one 4.1 KB row per frame; computed in
//                                 float64, stored rounded: the linear path's values are float32
//                                 already, the mel path's rounding moves the waveform ~1e-6)
//   frames [2][B][Fmax][WINP]     windowed inverse-FFT output of every frame, window support only
//                                 (WIN = 1102 samples; the padded Hann is zero elsewhere).  The
//                                 batched (unfused) loop stores them float32, rounded once before
//                                 librosa's float32 overlap-add (round 3: float64 slots were 2/3 of
//                                 its HBM traffic); the fused and persistent loops, which gather
//                                 every sample from its <= 5 contributing frames, keep float64 (their
//                                 sc1 4-byte gathers measured 2.4 -> 4.3 us per iteration)
// One workgroup per (sentence, frame) per iteration does the whole GL iteration for its frame:
//   overlap-add gather of the previous iteration's frames (<= 5 contributors per sample) with the
//   window-sum-square normalisation and the STFT's reflect padding -> window -> 2048-point real
//   FFT (1024-point complex Stockham radix-4 in LDS) -> S * X/|X| -> inverse real FFT -> window
//   -> store the frame.  Iterations ping-pong the frames buffer (a frame's neighbours still read
//   the previous iteration), one launch per iteration, replayed from a hipGraph.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "gl_fft.h"
#include "handoff.h"

#ifndef GLP_SLEEP
#define GLP_SLEEP 1  // persistent loop: s_sleep between neighbour-tag polls
#endif

using namespace tts;
using namespace tts::handoff;

namespace {

// a frame sample as float64 from its storage (gl_handle.h: frame_t, gran_t), and its store
__device__ __forceinline__ double fval(float x) { return (double)x; }
__device__ __forceinline__ double fval(gran_t x) { return (double)__uint_as_float((unsigned)x.v); }
__device__ __forceinline__ void fstore(float* p, double v, unsigned) { *p = (float)v; }
__device__ __forceinline__ void fstore(gran_t* p, double v, unsigned tag) {
    p->v = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint((float)v);
}

constexpr int MAG_KT = 64;  // magnitude kernel tile: bins (one per lane) ...
constexpr int MAG_FT = 16;  // ... x frames (MAG_FT / 4 per wave)
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_PER = 8;  // samples per thread per scan tile
constexpr int SCAN_CHUNK = 4096;  // de-emphasis output samples per workgroup

// LDS slot of complex point i in the fft1024_regs buffers: rows of 16 points (256 B, all 64
// banks) with the 16-byte columns XOR-swizzled by 5 * (row mod 4).  The Ns = 1 pass stores lane
// j's points at 4j + r (16 lanes span 4 rows, columns {0, 4, 8, 12}) and the Ns = 4 pass at
// 16 (j/4) + j%4 + 4r (4 rows, columns {0..3}): both land on 16 distinct columns instead of
// 4-way bank conflicts; contiguous reads stay a permutation of one row.
__device__ __forceinline__ int swz(int i) { return i ^ (5 * ((i >> 4) & 3)); }

// ---- two-level 1024-point complex FFT of one 256-thread workgroup (round 5).  1024 = 4 x 256:
// one radix-4 step ACROSS the four waves, thread-local in registers, and one 256-point Stockham
// radix-4 FFT per wave whose three LDS exchanges stay inside that wave's own 256-slot region.  A
// wave's LDS operations execute in issue order, so the wave-local exchanges need no barrier: the
// transform has ONE workgroup barrier (the cross-wave hand-over) instead of four.
//   layout A (thread t = 64 w + l):  v[r] = z[t + 256 r]          (edge_sample: STFT input, iSTFT output)
//   layout B (wave w, lane l):        v[r] = Z[4 (l + 64 r) + w]   (the spectrum's bins)
// Forward, decimation in frequency, A -> B:
//   u_q[m] = W1024^(m q) sum_s z[m + 256 s] W4^(s q)  (thread m: a butterfly over its registers),
//   Z[4 k1 + q] = sum_m u_q[m] W256^(m k1)            (wave q: 256-point FFT over m = l + 64 r);
// inverse, decimation in time, B -> A: the same two steps in reverse order with conjugate twiddles.
// Region q of a buffer is slots [256 q, 256 q + 256), points XOR-swizzled by swz (the Stockham
// store patterns of a 256-point pass are the first three of the 1024-point one).
// threadIdx.x through an opaque copy: LDS addresses derived from it are recomputed per transform
// instead of hoisted out of the persistent loop, where dozens of them would stay live (and spill)
__device__ __forceinline__ int tid_opaque() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
template <bool INV>
__device__ __forceinline__ void bfly4(double2 (&v)[4]) {
    const double2 a0 = double2{v[0].x + v[2].x, v[0].y + v[2].y};
    const double2 a1 = double2{v[0].x - v[2].x, v[0].y - v[2].y};
    const double2 a2 = double2{v[1].x + v[3].x, v[1].y + v[3].y};
    const double2 a3 = double2{v[1].x - v[3].x, v[1].y - v[3].y};
    // -i*a3 = (a3.y, -a3.x); +i*a3 = (-a3.y, a3.x)
    const double2 m3 = INV ? double2{-a3.y, a3.x} : double2{a3.y, -a3.x};
    v[0] = double2{a0.x + a2.x, a0.y + a2.y};
    v[1] = double2{a1.x + m3.x, a1.y + m3.y};
    v[2] = double2{a0.x - a2.x, a0.y - a2.y};
    v[3] = double2{a1.x - m3.x, a1.y - m3.y};
}
// Twiddles of the two-level FFT (entries of the 2048-point table tw[m] = W2048^m):
//   fx(q)     = W1024^(t q), q = 1..3            (forward cross-wave step, thread t)
//   ix(r)     = W1024^((l + 64 r) w)             (inverse cross-wave step, wave w, lane l)
//   ps(p, r)  = W_(4 Ns)^(r (l mod Ns)), r = 1..3 (wave pass p = 0, 1, 2: Ns = 4, 16, 64)
// TwRegs holds all 16 in registers for the kernel's lifetime (the persistent loop: one wave per
// SIMD, registers to spare); TwTable reads the L2-resident table where they are used (the
// register-budget forms).  Same values either way, so the forms are bitwise equal.
struct TwRegs {
    double2 f[3], i[4], p[3][3];
    __device__ __forceinline__ void load(const double2* __restrict__ tw) {
        const int t = threadIdx.x, l = t & 63, w = t >> 6;
#pragma unroll
        for (int q = 1; q < 4; ++q) f[q - 1] = tw[2 * t * q];
#pragma unroll
        for (int r = 0; r < 4; ++r) i[r] = tw[2 * (l + 64 * r) * w];
#pragma unroll
        for (int ps = 0; ps < 3; ++ps) {
            const int Ns = 4 << (2 * ps);
#pragma unroll
            for (int r = 1; r < 4; ++r) p[ps][r - 1] = tw[(l & (Ns - 1)) * r * (512 / Ns)];
        }
    }
    __device__ __forceinline__ double2 tw_at(int) const { return double2{0.0, 0.0}; }  // (TwTable only)
    __device__ __forceinline__ double2 fx(int q) const { return f[q - 1]; }
    __device__ __forceinline__ double2 ix(int r) const { return i[r]; }
    __device__ __forceinline__ double2 ps(int p_, int r) const { return p[p_][r - 1]; }
};
// TwMix (the two-per-CU persistent form's register budget): the forward cross-wave twiddles in
// registers, the wave passes' from a 252-entry LDS copy (pt: [pass][l mod Ns][r - 1], 4 KB), the
// inverse cross-wave ones from the table (fetched ahead of the wave FFT).
constexpr int TW_LDS = 3 * (4 + 16 + 64);
__device__ __forceinline__ int tw_lds_base(int p_) { return p_ == 0 ? 0 : p_ == 1 ? 12 : 60; }
typedef __attribute__((address_space(1))) const double g_d;  // global
typedef __attribute__((address_space(3))) const double l_d;  // LDS
struct TwMix {
    g_d* tw;  // (address-space-qualified scalars: the table reads stay global / LDS loads)
    l_d* pt;
    double2 f[3];
    __device__ __forceinline__ void load(const double2* __restrict__ t) {
        const int j = threadIdx.x;
        tw = (g_d*)t;
#pragma unroll
        for (int q = 1; q < 4; ++q) f[q - 1] = t[2 * j * q];
    }
    // fill the LDS copy (every thread; the caller's barrier orders it before the first use)
    __device__ __forceinline__ static void fill(double2* lds, const double2* __restrict__ t) {
        for (int e = threadIdx.x; e < TW_LDS; e += blockDim.x) {
            const int p_ = e < 12 ? 0 : e < 60 ? 1 : 2, o = e - tw_lds_base(p_);
            const int Ns = 4 << (2 * p_), k = o / 3, r = o % 3 + 1;
            lds[e] = t[k * r * (512 / Ns)];
        }
    }
    __device__ __forceinline__ double2 tw_at(int k) const { return double2{tw[2 * k], tw[2 * k + 1]}; }
    __device__ __forceinline__ double2 fx(int q) const { return f[q - 1]; }
    __device__ __forceinline__ double2 ix(int r) const {
        return tw_at(2 * (((int)threadIdx.x & 63) + 64 * r) * ((int)threadIdx.x >> 6));
    }
    __device__ __forceinline__ double2 ps(int p_, int r) const {
        const int Ns = 4 << (2 * p_), e = tw_lds_base(p_) + ((int)threadIdx.x & (Ns - 1)) * 3 + r - 1;
        return double2{pt[2 * e], pt[2 * e + 1]};
    }
};
struct TwTable {
    const double2* __restrict__ tw;
    __device__ __forceinline__ double2 tw_at(int k) const { return tw[k]; }
    __device__ __forceinline__ double2 fx(int q) const { return tw[2 * (int)threadIdx.x * q]; }
    __device__ __forceinline__ double2 ix(int r) const {
        return tw[2 * (((int)threadIdx.x & 63) + 64 * r) * ((int)threadIdx.x >> 6)];
    }
    __device__ __forceinline__ double2 ps(int p_, int r) const {
        const int Ns = 4 << (2 * p_);
        return tw[((int)threadIdx.x & (Ns - 1)) * r * (512 / Ns)];
    }
};

// 256-point Stockham radix-4 FFT of one wave, in place in its region rg: enters with v[r] =
// u[l + 64 r] (the first pass's operands, so it reads no LDS), leaves v[r] = U[l + 64 r] (the last
// pass's outputs stay in registers).  Each pass's twiddles are fetched one pass ahead.
template <bool INV, class TW>
__device__ __forceinline__ void wave_fft256(double2 (&v)[4], double2* rg, int l, const TW& tw) {
    asm volatile("" : "+v"(l));
    double2 w[3];
#pragma unroll
    for (int r = 1; r < 4; ++r) w[r - 1] = tw.ps(0, r);
#pragma unroll
    for (int p = -1; p < 3; ++p) {
        const int Ns = 1 << (2 * (p + 1));
        if (p >= 0) {
            double2 wn[3];
            if (p < 2) {
#pragma unroll
                for (int r = 1; r < 4; ++r) wn[r - 1] = tw.ps(p + 1, r);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = rg[swz(l + 64 * r)];
#pragma unroll
            for (int r = 1; r < 4; ++r) v[r] = cmul(v[r], INV ? cconj(w[r - 1]) : w[r - 1]);
            if (p < 2) {
#pragma unroll
                for (int r = 0; r < 3; ++r) w[r] = wn[r];
            }
        }
        bfly4<INV>(v);
        if (p == 2) return;  // Ns = 64: lane l's outputs are U[l + 64 r]
        const int idxD = (l / Ns) * Ns * 4 + (l & (Ns - 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) rg[swz(idxD + r * Ns)] = v[r];
        __builtin_amdgcn_wave_barrier();  // (code motion only: the wave's LDS ops run in order)
    }
}
// Forward two-level FFT, layout A -> B.  Writes every region of wr (the caller's earlier readers
// of wr must be past a barrier); one barrier.
template <class TW>
__device__ __forceinline__ void fft2l_fwd(double2 (&v)[4], double2* wr, const TW& tw) {
    const int t = tid_opaque(), l = t & 63, w = threadIdx.x >> 6;
    bfly4<false>(v);
#pragma unroll
    for (int q = 1; q < 4; ++q) v[q] = cmul(v[q], tw.fx(q));
#pragma unroll
    for (int q = 0; q < 4; ++q) wr[256 * q + swz(t)] = v[q];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = wr[256 * w + swz(l + 64 * r)];
    wave_fft256<false>(v, wr + 256 * w, l, tw);
}
// Inverse two-level FFT, layout B -> A (unnormalised).  Uses region w of wr first (the caller's
// earlier readers of that region must be past a barrier), then reads every region; one barrier.
template <class TW>
__device__ __forceinline__ void fft2l_inv(double2 (&v)[4], double2* wr, const TW& tw) {
    const int t = tid_opaque(), l = t & 63, w = threadIdx.x >> 6;
    double2* rg = wr + 256 * w;
    double2 iw[4];  // (fetched ahead of the wave FFT: in flight during it when read from the table)
#pragma unroll
    for (int r = 0; r < 4; ++r) iw[r] = tw.ix(r);
    wave_fft256<true>(v, rg, l, tw);
    if (w != 0) {  // (wave 0's twiddles are 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = cmul(v[r], cconj(iw[r]));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) rg[swz(l + 64 * r)] = v[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = wr[256 * q + swz(t)];
    bfly4<true>(v);
}

// Bin k of the thread's register r in layout B
__device__ __forceinline__ int bin2l(int t, int r) { return 4 * ((t & 63) + 64 * r) + (t >> 6); }
__device__ __forceinline__ int bin2l(int r) { return bin2l((int)threadIdx.x, r); }
// STFT value of bin k from zk = Z[k mod 1024] and zm = Z[(1024 - k) mod 1024] (real-FFT split),
// rounded to complex64 (librosa stft dtype), then |S| exp(i angle X) (angle(0) = 0) in float64
// (utils/audio.py:187-188) by one reciprocal square root (the float-rounded components square
// exactly in double): no divisions on the iteration's critical path.  Im = 0 at DC and Nyquist
// (istft: .real of the Hermitian extension).
__device__ __forceinline__ double2 spec_bin(double2 zk, double2 zm, double2 t, double s, bool edge) {
    const double2 zc = cconj(zm);
    const double2 E = double2{0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y)};
    const double2 O = double2{0.5 * (zk.y - zc.y), -0.5 * (zk.x - zc.x)};  // -i (zk - zc) / 2
    const double xre = (double)(float)(E.x + (t.x * O.x - t.y * O.y));
    const double xim = (double)(float)(E.y + (t.x * O.y + t.y * O.x));
    const double m2 = xre * xre + xim * xim;
    // the hardware reciprocal square root (~2^-23) and one Newton step (~2^-45): the reference's
    // unit phase is itself complex64 (np.exp(1j * np.angle(X)) on a complex64 X)
    double ri = __builtin_amdgcn_rsq(m2);
    ri = fma(0.5 * ri, fma(-m2 * ri, ri, 1.0), ri);
    double2 xv = m2 > 0.0 ? double2{s * (xre * ri), s * (xim * ri)} : double2{s, 0.0};
    if (edge) xv.y = 0.0;
    return xv;
}
// Forward spectrum step in layout B: v = Z on entry, X = |S| X/|X| on return; the Nyquist bin
// X[1024] goes to xnyq of thread 0 (wave 0, lane 0: it holds Z[0] and is the only reader of
// X[1024]).  zb: 1024 slots (one barrier after the Z stores; the caller's earlier readers of zb
// must be past a barrier).  tk(r) = W2048^k and sk(r) = |S|[k] for the thread's bins k = bin2l(r);
// tnyq / snyq: the same for k = 1024 (thread 0).
template <class TK, class SK>
__device__ __forceinline__ void spectrum2l(double2 (&v)[4], double2* zb, TK tk, SK sk, double2 tnyq, double snyq,
                                           double2& xnyq) {
    const int t = tid_opaque();
#pragma unroll
    for (int r = 0; r < 4; ++r) zb[swz(bin2l(t, r))] = v[r];
    __syncthreads();
    if (threadIdx.x == 0) xnyq = spec_bin(v[0], v[0], tnyq, snyq, true);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = bin2l(t, r);
        v[r] = spec_bin(v[r], zb[swz((NH - k) & (NH - 1))], tk(r), sk(r), k == 0);
    }
}
// Inverse real-FFT pre-split in layout B: v = X on entry, z'[k] = E + i O on return
// (E = (X[k] + conj X[N-k]) / 2, O = (X[k] - conj X[N-k]) / 2 * conj(t)); xb: 1024 slots (one
// barrier after the X stores; the caller's earlier readers of xb must be past a barrier).
template <class TK>
__device__ __forceinline__ void presplit2l(double2 (&v)[4], double2* xb, TK tk, double2 xnyq) {
    const int t = tid_opaque();
#pragma unroll
    for (int r = 0; r < 4; ++r) xb[swz(bin2l(t, r))] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = bin2l(t, r);
        const double2 xk = v[r];
        double2 xm = xb[swz((NH - k) & (NH - 1))];
        if (r == 0 && k == 0) xm = xnyq;  // (bin 0 pairs with the Nyquist bin: thread 0, register 0)
        const double2 xc = cconj(xm);
        const double2 E = double2{0.5 * (xk.x + xc.x), 0.5 * (xk.y + xc.y)};
        const double2 D = double2{0.5 * (xk.x - xc.x), 0.5 * (xk.y - xc.y)};
        const double2 O = cmul(D, cconj(tk(r)));
        v[r] = double2{E.x - O.y, E.y + O.x};  // E + i O
    }
}

// Real sample i (0..7) of thread j in layout A (fft2l_fwd's input, fft2l_inv's output): complex point j + 256 (i/2),
// real part (i even) or imaginary part (i odd) = real sample 2 j + 512 (i/2) + (i & 1).
__device__ __forceinline__ int edge_sample(int j, int i) { return 2 * j + 512 * (i >> 1) + (i & 1); }

// Bijective XCD-aware remap: consecutive logical frames share an XCD (their OLA gathers
// re-read each other's frames through that XCD's L2).  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int n) {
    const int q = n >> 3, r = n & 7, x = bid & 7, i = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}


// float32 y[p] of the previous iteration's iSTFT (librosa istft): float64 frame contributions
// added frame by frame into a float32 accumulator, divided (float32) by the float32 window
// sum-square where it exceeds float32 tiny.  q = p + n_fft/2 is the untrimmed position.
template <typename FT>
__device__ __forceinline__ float ola_sample(const FT* __restrict__ fr, int q, int F, const Geo& g,
                                            const double* __restrict__ win2) {
    if (q < g.woff) return 0.f;
    int ilo = q - g.woff - g.win + 1;
    ilo = ilo <= 0 ? 0 : (ilo + g.hop - 1) / g.hop;
    int ihi = (q - g.woff) / g.hop;
    if (ihi > F - 1) ihi = F - 1;
    float y = 0.f, wss = 0.f;
    for (int i = ilo; i <= ihi; ++i) {
        const int o = q - i * g.hop;  // offset inside frame i (0..2047)
        y = (float)((double)y + fval(fr[(int64_t)i * g.winp + (o - g.fb)]));
        wss = (float)((double)wss + win2[o]);
    }
    return wss > 1.17549435e-38f ? y / wss : y;
}

// ola_sample with the <= OLA_MAX contributing frames' loads issued together (the sum still runs
// frame by frame in index order; absent contributors add exact zeros): bitwise equal to it.
constexpr int OLA_MAX = 5;  // ceil(win / hop) for the reference geometry (1102 / 275)
template <typename FT>
__device__ __forceinline__ float ola_sample_unrolled(const FT* __restrict__ fr, int q, int F, const Geo& g,
                                                     const double* __restrict__ win2) {
    if (q < g.woff) return 0.f;
    int ilo = q - g.woff - g.win + 1;
    ilo = ilo <= 0 ? 0 : (ilo + g.hop - 1) / g.hop;
    int ihi = (q - g.woff) / g.hop;
    if (ihi > F - 1) ihi = F - 1;
    double fv[OLA_MAX], wv[OLA_MAX];
#pragma unroll
    for (int k = 0; k < OLA_MAX; ++k) {
        const int i = ilo + k;
        const int o = q - i * g.hop;
        const bool ok = i <= ihi;
        fv[k] = ok ? fval(fr[(int64_t)i * g.winp + (o - g.fb)]) : 0.0;
        wv[k] = ok ? win2[o] : 0.0;
    }
    float y = 0.f, wss = 0.f;
#pragma unroll
    for (int k = 0; k < OLA_MAX; ++k) {
        y = (float)((double)y + fv[k]);
        wss = (float)((double)wss + wv[k]);
    }
    return wss > 1.17549435e-38f ? y / wss : y;
}

// ---------------------------------------------------------------- |S|^power
struct MagArgs {
    int mode;  // TTS_GL_FROM_MEL / TTS_GL_FROM_LINEAR
    const float* spec;
    int n_in, Fmax;
    const int* F;
    const double* pinv;  // [n_mels][1025]: pinv(mel basis) transposed (lanes read consecutive bins)
    spec_t* S;
    float min_db, ref_db, power, max_norm;
    int signal_norm, symmetric, clip;
};

// _denormalize (utils/audio.py:96-112) then the exponent of _db_to_amp(x + ref_level_db)
// (:125-126), in float32 as numpy computes them on the float32 network output.
__device__ __forceinline__ float denorm_db(float x, const MagArgs& a) {
    float d = x;
    if (a.signal_norm) {
        if (a.symmetric) {
            if (a.clip) d = fminf(fmaxf(d, -a.max_norm), a.max_norm);
            d = ((d + a.max_norm) * -a.min_db / (2.f * a.max_norm)) + a.min_db;
        } else {
            if (a.clip) d = fminf(fmaxf(d, 0.f), a.max_norm);
            d = (d * -a.min_db / a.max_norm) + a.min_db;
        }
    }
    return (d + a.ref_db) * 0.05f;
}
// the amplitude 10^e: powf (the mel path: 80 values per frame) or exp10f (the linear path: 1025)
__device__ __forceinline__ float denorm_to_amp(float x, const MagArgs& a) { return powf(10.f, denorm_db(x, a)); }
__device__ __forceinline__ float amp_of_db(float x, const MagArgs& a) { return exp10f(denorm_db(x, a)); }

// inv_spectrogram's |S|: S (float32) ** power in float32, then widened (utils/audio.py:156-160).
// The two float32 steps as numpy has them, each within an ulp or two of its powf: the amplitude
// 10^e by exp10f, and power 1.5 (the reference configs) as a * sqrt(a).  A streaming launch with
// no LDS, LIN_PER elements per thread (round 4's tile launch with two powf per bin: 788 us at
// configs[4], dispatch- and VALU-bound).
constexpr int LIN_PER = 16;
__global__ __launch_bounds__(256) void gl_linear_magnitude_kernel(const MagArgs a) {
    const int b = blockIdx.y;
    const int64_t n = (int64_t)a.F[b] * NB;  // the sentence's frames < F[b], each a 1025-bin row
    const int64_t base = (int64_t)blockIdx.x * (256 * LIN_PER) + threadIdx.x;
    if (base >= n) return;
    const float* sp = a.spec + (int64_t)b * a.Fmax * NB;
    spec_t* S = a.S + (int64_t)b * a.Fmax * NB;
    float x[LIN_PER];
#pragma unroll
    for (int i = 0; i < LIN_PER; ++i) {
        const int64_t e = base + i * 256;
        x[i] = e < n ? sp[e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < LIN_PER; ++i) {
        const int64_t e = base + i * 256;
        const float amp = amp_of_db(x[i], a);
        if (e < n) S[e] = (spec_t)(a.power == 1.5f ? amp * sqrtf(amp) : powf(amp, a.power));
    }
}

// Tile = MAG_KT bins x MAG_FT frames per workgroup: the pinv columns of the tile's bins staged in
// LDS once, the frames' amplitudes (float, as numpy has them) computed into LDS, then lane = bin,
// each wave MAG_FT / 4 frames, every (bin, frame) dot product summed over mels in order.
__global__ __launch_bounds__(256) void gl_magnitude_kernel(const MagArgs a) {
    const int b = blockIdx.z;
    const int Fb = a.F[b];
    const int f0 = blockIdx.y * MAG_FT;
    if (f0 >= Fb) return;
    const int nf = min(MAG_FT, Fb - f0);
    const float* sp = a.spec + ((int64_t)b * a.Fmax + f0) * a.n_in;
    spec_t* S = a.S + ((int64_t)b * a.Fmax + f0) * NB;
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * MAG_KT;
    __shared__ double pw[80][MAG_KT];
    __shared__ float amp[MAG_FT][80];
    // fixed trip counts (n_in <= 80): every staging load of the tile is in flight at once
    constexpr int PWL = 80 * MAG_KT / 256, AML = MAG_FT * 80 / 256;
    double pv[PWL];
    float sv[AML];
#pragma unroll
    for (int j = 0; j < PWL; ++j) {
        const int i = tid + j * 256, m = i / MAG_KT, kk = i % MAG_KT;
        pv[j] = m < a.n_in && k0 + kk < NB ? a.pinv[(int64_t)m * NB + k0 + kk] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < AML; ++j) {
        const int i = tid + j * 256, f = i / 80, m = i % 80;
        sv[j] = f < nf && m < a.n_in ? sp[f * a.n_in + m] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < PWL; ++j) {
        const int i = tid + j * 256;
        pw[i / MAG_KT][i % MAG_KT] = pv[j];
    }
#pragma unroll
    for (int j = 0; j < AML; ++j) {
        const int i = tid + j * 256, f = i / 80, m = i % 80;
        amp[f][m] = f < nf && m < a.n_in ? denorm_to_amp(sv[j], a) : 0.f;
    }
    __syncthreads();
    // _mel_to_linear: max(1e-10, pinv(M) . S) in float64 (utils/audio.py:64-66), then ** power
    const int lane = tid & 63, wave = tid >> 6, k = k0 + lane;
    constexpr int FW = MAG_FT / 4;
    double acc[FW];
#pragma unroll
    for (int i = 0; i < FW; ++i) acc[i] = 0.0;
    // a fixed trip count (n_in <= 80: the staged rows past n_in are zeros, whose products add +0.0)
    // keeps the LDS reads in flight ahead of the FMAs
#pragma unroll 8
    for (int m = 0; m < 80; ++m) {
        const double w = pw[m][lane];
#pragma unroll
        for (int i = 0; i < FW; ++i) acc[i] += w * (double)amp[wave * FW + i][m];
    }
    if (k < NB) {
#pragma unroll
        for (int i = 0; i < FW; ++i) {
            const int f = wave * FW + i;
            if (f < nf) {
                // power 1.5 (the reference configs): x * sqrt(x), within an ulp of pow in float64
                // and far below the float32 rounding of the stored value; else pow
                const double x = fmax(acc[i], 1e-10);
                S[(int64_t)f * NB + k] = (spec_t)(a.power == 1.5f ? x * sqrt(x) : pow(x, (double)a.power));
            }
        }
    }
}

// ---------------------------------------------------------------- GL iteration
__device__ __forceinline__ double hash_uniform(unsigned long long seed, unsigned long long idx) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// FUSED (small batches): the frame's own 2048 STFT input samples are overlap-added from the
// previous iteration's frames inside this launch (bitwise the values gl_ola_kernel would store),
// so an iteration is one launch instead of two.
template <bool INIT, bool FUSED, typename FT>
// Four workgroups per CU (32 KB of LDS, <= 128 VGPRs each).  Measured at B = 64: the same speed
// as three workgroups with the FFT twiddles held in registers, faster than five (which spill).
__global__ __launch_bounds__(GL_THREADS, 4) void gl_iter_kernel(const IterArgs a) {
    const int b = blockIdx.y;
    const int f = xcd_remap(blockIdx.x, gridDim.x);
    const int Fb = a.F[b];
    // the persistent loop's status word is cleared by block (0, 0) even when the run is empty
    // (a speculative batch-1 run whose frame count was clamped to 0): its final overlap-add launch
    // copies the word to the host, which must not see an earlier run's failure
    if (INIT && a.zero_status && threadIdx.x == 0 && (blockIdx.x | blockIdx.y) == 0) *a.zero_status = 0;
    if (f >= Fb) return;
    const Geo g = a.g;
    const int tid = threadIdx.x;
    if (INIT && tid == 0 && a.zero_flags)  // the persistent loop that follows reads tags of frames < F[b] only
        a.zero_flags[(int64_t)b * a.Fmax + f] = 0u;
    __shared__ __align__(16) double2 buf0[NH];  // forward wave regions, then the spectrum X
    __shared__ __align__(16) double2 buf1[NH];  // Z, then the inverse wave regions
    // (the Nyquist bin X[1024] stays in a register of thread 0, its only writer and reader)
    double2 xnyq = double2{0.0, 0.0};
    const TwTable twt{a.c.tw};
    const spec_t* Sf = a.S + ((int64_t)b * a.Fmax + f) * NB;
    // ---- phase 0: the frame's global operands are issued before anything waits: window, |S|,
    // the input samples (the FFT and split twiddles, an L2-resident table, are read where used:
    // holding them across the forward FFT would cost a wave per SIMD)
    constexpr int PN = NFFT / GL_THREADS;  // samples per thread (8)
    // |S| of the thread's bins k = bin2l(r) (layout B), and of the Nyquist bin on thread 0
    double sk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sk[r] = (double)Sf[bin2l(r)];
    const double snyq = tid == 0 ? (double)Sf[NH] : 0.0;
    // the padded Hann at this thread's samples: the analysis window of the STFT input (the
    // forward FFT's layout-A registers) and the synthesis window of the iSTFT output (the inverse
    // FFT's, layout A again) sit at the same sample indices
    double wo[PN];
#pragma unroll
    for (int i = 0; i < PN; ++i) {
        const int m = edge_sample(tid, i), n = m - g.woff;
        wo[i] = n >= 0 && n < g.win ? a.c.win[m] : 0.0;
    }
    double2 v[4];
    if (!INIT) {
        // ---- STFT frame f of the previous iteration's float32 signal (librosa stft, centre reflect pad)
        const int N = g.hop * (Fb - 1);
        const float* yb = a.y + (int64_t)b * a.Nmax;
        float yi[PN];
#pragma unroll
        for (int i = 0; i < PN; ++i) {
            const int n = edge_sample(tid, i);  // the forward FFT's operands stay in registers
            const bool sup = n >= g.woff && n < g.woff + g.win;  // the padded Hann's support
            if (FUSED) {
                const FT* fb = static_cast<const FT*>(a.prev) + (int64_t)b * a.Fmax * g.winp;
                yi[i] = sup ? ola_sample_unrolled(fb, reflect_idx(f * g.hop + n - NFFT / 2, N) + NFFT / 2, Fb, g, a.c.win2)
                            : 0.f;
            } else {
                yi[i] = sup ? yb[reflect_idx(f * g.hop + n - NFFT / 2, N)] : 0.f;
            }
        }
        // z[n] = x[2n] + i x[2n+1] == real x[0..2047]
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = double2{wo[2 * r] * (double)yi[2 * r], wo[2 * r + 1] * (double)yi[2 * r + 1]};
        fft2l_fwd(v, buf0, twt);
        spectrum2l(v, buf1, [&](int r) { return a.c.tw[bin2l(r)]; }, [&](int r) { return sk[r]; }, a.c.tw[NH], snyq,
                   xnyq);
    } else {
        // ---- initial phases exp(2 pi i U), U ~ U[0,1)  (utils/audio.py:183), per bin of layout B
        auto init_bin = [&](int k, double sv) {
            const double u = a.phase_u ? a.phase_u[((int64_t)b * NB + k) * a.Fmax + f]
                                       : hash_uniform(a.seed, ((unsigned long long)b * NB + k) * 1048576ull + f);
            double sn, cs;
            sincospi(2.0 * u, &sn, &cs);  // (exp(2 pi i u) without rounding 2 pi u first)
            return double2{sv * cs, (k == 0 || k == NB - 1) ? 0.0 : sv * sn};
        };
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = init_bin(bin2l(r), sk[r]);
        if (tid == 0) xnyq = init_bin(NH, snyq);
    }
    // ---- inverse real FFT (istft: ifft of the Hermitian-extended spectrum, .real => Im X_0 =
    // Im X_N/2 = 0, set where X is formed)
    presplit2l(v, buf0, [&](int r) { return a.c.tw[bin2l(r)]; }, xnyq);
    fft2l_inv(v, buf1, twt);
    // ---- window and store the support [woff, woff+win) in float64 (ytmp of librosa istft), from
    // the inverse FFT's registers
    FT* out = static_cast<FT*>(a.next) + ((int64_t)b * a.Fmax + f) * g.winp;
#pragma unroll
    for (int i = 0; i < PN; ++i) {
        const int n = edge_sample(tid, i) - g.woff;
        const double zv = (i & 1) ? v[i >> 1].y : v[i >> 1].x;
        if (n >= 0 && n < g.win) fstore(out + (n + g.woff - g.fb), wo[i] * (zv * (1.0 / NH)), a.gtag);
    }
}

// ---------------------------------------------------------------- GL iteration, one wave per frame
// The batched form of gl_iter_kernel<false, false> (same inputs: the previous iteration's float32
// signal; same output: the windowed float64 frame), with each frame's whole iteration on ONE
// wave: the 1024-point complex FFT as radix 16 x 16 x 4 with 16 points per lane in registers and
// two wave-local LDS transposes per FFT, so no pass waits on a workgroup barrier and every
// butterfly's operands stay in VGPRs.  Index map (lane L, register r):
//   pass 1:  z[L + 64 r]                     radix-16 over r, x W1024^(L k2)
//   pass 2:  lane p1 + 4 k2, register p2     radix-16 over p2, x W64^(p1 q2)
//   pass 3:  lane r3 + 4 k2, register 4j+p1  radix-4 over p1
//   output:  lane r3 + 4 k2, register 4j+q1 holds Z[256 q1 + 64 j + 16 r3 + k2]
// The real-FFT split, the phase step and the inverse pre-split run per bin pair (k, 1024 - k) in
// the lane that owns k in the pass-1 layout of the inverse FFT; the partner's pre-split value moves
// to its owner lane (64 - L) through LDS.  LDS slots are XOR-swizzled so every exchange is free of
// bank conflicts (ds_write_b128 8-lane groups, ds_read_b128 16-lane groups).
// Twiddles: wt[k2][L] = W1024^(L k2) and wt[16 + q2][L] = W64^((L & 3) q2) (host-built, f64).
constexpr int WV_SLOTS = NH + 1;  // LDS complex slots per wave (the Nyquist bin at slot 1024)

// W32^m = e^{-i pi m / 16}, m < 8 (the split twiddle steps of the bin-pair loop)
__device__ constexpr double kW32[8][2] = {
    {1.00000000000000000000, -0.00000000000000000000},
    {0.98078528040323043058, -0.19509032201612824808},
    {0.92387953251128673848, -0.38268343236508978178},
    {0.83146961230254523567, -0.55557023301960217765},
    {0.70710678118654757274, -0.70710678118654746172},
    {0.55557023301960228867, -0.83146961230254523567},
    {0.38268343236508983729, -0.92387953251128673848},
    {0.19509032201612833135, -0.98078528040323043058}};

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ double2 cmulf(double2 a, double2 w) {  // a * w
    return double2{fma(a.x, w.x, -(a.y * w.y)), fma(a.x, w.y, a.y * w.x)};
}
__device__ __forceinline__ double2 cmulcf(double2 a, double2 w) {  // a * conj(w)
    return double2{fma(a.x, w.x, a.y * w.y), fma(a.y, w.x, -(a.x * w.y))};
}
template <bool INV>
__device__ __forceinline__ double2 rotq(double2 a) {  // a * (-i) forward, a * (+i) inverse
    return INV ? double2{-a.y, a.x} : double2{a.y, -a.x};
}
template <bool INV>
__device__ __forceinline__ void dft4(double2& a0, double2& a1, double2& a2, double2& a3) {
    const double2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = rotq<INV>(csub(a1, a3));
    a0 = cadd(t0, t2);
    a1 = cadd(t1, t3);
    a2 = csub(t0, t2);
    a3 = csub(t1, t3);
}
// a * W16^E (E in 1..9; the inverse uses conj(W16^E))
template <int E, bool INV>
__device__ __forceinline__ double2 tw16(double2 a) {
    constexpr double C1 = 0.92387953251128675613, S1 = 0.38268343236508977173, C2 = 0.70710678118654752440;
    if constexpr (E == 4) return rotq<INV>(a);
    if constexpr (E == 2) {  // (1 - i) / sqrt 2
        return INV ? double2{C2 * (a.x - a.y), C2 * (a.x + a.y)} : double2{C2 * (a.x + a.y), C2 * (a.y - a.x)};
    }
    if constexpr (E == 6) {  // (-1 - i) / sqrt 2
        return INV ? double2{-C2 * (a.x + a.y), C2 * (a.x - a.y)} : double2{C2 * (a.y - a.x), -C2 * (a.x + a.y)};
    }
    constexpr double wr = E == 1 ? C1 : E == 3 ? S1 : -C1;  // E = 1, 3, 9
    constexpr double wi = E == 1 ? -S1 : E == 3 ? -C1 : S1;
    return INV ? cmulcf(a, double2{wr, wi}) : cmulf(a, double2{wr, wi});
}
// in-register 16-point DFT: v[n] -> v[k] (natural order), as 4 x 4 with W16 twiddles
template <bool INV>
__device__ __forceinline__ void dft16(double2 (&v)[16]) {
#pragma unroll
    for (int n1 = 0; n1 < 4; ++n1) dft4<INV>(v[n1], v[n1 + 4], v[n1 + 8], v[n1 + 12]);  // k2 at v[n1 + 4 k2]
    v[5] = tw16<1, INV>(v[5]);
    v[9] = tw16<2, INV>(v[9]);
    v[13] = tw16<3, INV>(v[13]);
    v[6] = tw16<2, INV>(v[6]);
    v[10] = tw16<4, INV>(v[10]);
    v[14] = tw16<6, INV>(v[14]);
    v[7] = tw16<3, INV>(v[7]);
    v[11] = tw16<6, INV>(v[11]);
    v[15] = tw16<9, INV>(v[15]);
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) dft4<INV>(v[4 * k2], v[4 * k2 + 1], v[4 * k2 + 2], v[4 * k2 + 3]);  // X[4 k1 + k2] at v[4 k2 + k1]
    double2 o[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) o[4 * k1 + k2] = v[4 * k2 + k1];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = o[i];
}
// LDS slots (8-byte words; every exchange moves real parts, then imaginary parts, through one
// 1025-word buffer).  Bank rules: ds_write_b64 in 16-lane contiguous groups over 32 banks,
// ds_read_b64 in 32-lane halves over 64 banks; these swizzles keep every exchange conflict-free.
__device__ __forceinline__ int wv_a1(int k2, int n1) { return k2 * 64 + (n1 ^ (4 * (k2 & 7))); }
__device__ __forceinline__ int wv_a2(int k2, int p1, int q2) { return k2 * 64 + 4 * (q2 ^ (k2 & 7)) + (p1 ^ (k2 & 3)); }
__device__ __forceinline__ int wv_sig(int k) { return k ^ (((k >> 4) & 3) << 2); }

// All-to-all of one wave's 16 complex registers through `lds`: real parts, then imaginary parts.
// Each round overwrites only registers whose value has already been stored (the real parts are
// read back into the real halves after every lane stored them), so 8 KB of LDS suffice.
template <class WS, class RS>
__device__ __forceinline__ void wave_xchg(double2 (&v)[16], double* lds, WS wslot, RS rslot) {
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[wslot(r)] = v[r].x;
    __syncthreads();  // one wave per workgroup: orders the lanes' LDS writes before the reads
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r].x = lds[rslot(r)];
    __syncthreads();  // the imaginary stores below do not depend on these reads
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[wslot(r)] = v[r].y;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r].y = lds[rslot(r)];
}

// 1024-point complex FFT of one wave (forward: e^{-i}, inverse: e^{+i}, unnormalised).
// In: v[r] = z[L + 64 r].  Out: v[4 j + q1] = Z[256 q1 + 64 j + 16 (L & 3) + (L >> 2)].
// Twiddles: pass 1 multiplies register k2 by w^k2, w = W1024^L (one load), the powers built by a
// product tree (depth <= 4, a few ulp); pass 2 reads W64^(p1 q2) from the wave's 64-entry LDS
// table t2[q2][p1] (4 distinct addresses per read).  The vector-memory path was the bound.
// Ends after a barrier that follows the last LDS reads.
template <bool INV>
__device__ __forceinline__ void wave_fft1024(double2 (&v)[16], double* lds, const double2* t2, __amdgpu_buffer_rsrc_t tw,
                                             int lane) {
    // the lane index is laundered per call: otherwise the inverse FFT reuses the forward's loads
    // and LDS addresses, which then stay live (and spill) across the spectrum step
    int L = lane;
    asm volatile("" : "+v"(L));
    const double2 w1 = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(tw, 32 * L, 0, 0));
    dft16<INV>(v);
    {
        auto mul = [&](double2 a, double2 w) { return INV ? cmulcf(a, w) : cmulf(a, w); };
        const double2 w2 = cmulf(w1, w1), w4 = cmulf(w2, w2), w8 = cmulf(w4, w4);
        const double2 w3 = cmulf(w2, w1), w12 = cmulf(w8, w4);
        v[1] = mul(v[1], w1);
        v[2] = mul(v[2], w2);
        v[3] = mul(v[3], w3);
        v[4] = mul(v[4], w4);
        v[5] = mul(v[5], cmulf(w4, w1));
        v[6] = mul(v[6], cmulf(w4, w2));
        v[7] = mul(v[7], cmulf(w4, w3));
        v[8] = mul(v[8], w8);
        v[9] = mul(v[9], cmulf(w8, w1));
        v[10] = mul(v[10], cmulf(w8, w2));
        v[11] = mul(v[11], cmulf(w8, w3));
        v[12] = mul(v[12], w12);
        v[13] = mul(v[13], cmulf(w12, w1));
        v[14] = mul(v[14], cmulf(w12, w2));
        v[15] = mul(v[15], cmulf(w12, w3));
    }
    const int p1 = L & 3, K2 = L >> 2;
    wave_xchg(v, lds, [&](int k2) { return wv_a1(k2, L); }, [&](int p2) { return wv_a1(K2, p1 + 4 * p2); });
    dft16<INV>(v);
#pragma unroll
    for (int q2 = 1; q2 < 16; ++q2) {
        const double2 w = t2[q2 * 4 + p1];
        v[q2] = INV ? cmulcf(v[q2], w) : cmulf(v[q2], w);
    }
    __syncthreads();  // the previous exchange's last reads are done before this one's stores
    wave_xchg(v, lds, [&](int q2) { return wv_a2(K2, p1, q2); },
              [&](int r) { return wv_a2(K2, r & 3, 4 * (r >> 2) + p1); });
#pragma unroll
    for (int j = 0; j < 4; ++j) dft4<INV>(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    __syncthreads();
}

// STFT value X (rounded to complex64, librosa stft dtype) -> |S| X / |X| (angle(0) = 0).  The
// reference's unit phase is itself complex64 (np.exp(1j * np.angle(X)) on a complex64 X), so the
// hardware reciprocal square root plus one Newton step (relative error far below float32's) is
// ample; X may carry any power-of-two scale (the result does not).  |X|^2 of two floats is
// within fp64 range, so no operand scaling is needed.
__device__ __forceinline__ double2 unit_phase(double2 X, double s) {
    const double xre = (double)(float)X.x, xim = (double)(float)X.y;
    const double m2 = fma(xre, xre, xim * xim);
    double r = __builtin_amdgcn_rsq(m2);
    r = fma(0.5 * r, fma(-m2 * r, r, 1.0), r);
    const double sr = s * r;  // (|S| folded into the reciprocal: one product per component)
    return m2 > 0.0 ? double2{xre * sr, xim * sr} : double2{s, 0.0};
}
// inverse real-FFT pre-split, times 2: z'[k] = E + i O, 2E = X[k] + conj X[N-k],
// 2O = (X[k] - conj X[N-k]) * conj(t) (the factor 1/2 is folded into the output scale)
__device__ __forceinline__ double2 inv_presplit2(double2 xk, double2 xm, double2 t) {
    const double2 E = double2{xk.x + xm.x, xk.y - xm.y};
    const double2 D = double2{xk.x - xm.x, xk.y + xm.y};
    const double2 O = cmulcf(D, t);
    return double2{E.x - O.y, E.y + O.x};
}

// buffer-resource access (SGPR base + 32-bit lane offset; out-of-range loads read 0, stores drop)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float buf_f32(__amdgpu_buffer_rsrc_t r, int voff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}
__device__ __forceinline__ float buf_f32s(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ double buf_f64(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ double2 buf_c64(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ void buf_st_f64(double v, __amdgpu_buffer_rsrc_t r, int voff) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, 0, 0);
}

// INIT: the initial iSTFT of exp(2 pi i U) |S| (utils/audio.py:183) on the same wave layout: no
// STFT, the bin pairs' X formed from the phases, then the inverse half as below (the batched
// loops' first launch; the 256-thread gl_iter_kernel<true> took ~1.5x a wave iteration).
template <bool INIT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void gl_iter_wave_kernel(const IterArgs a) {
    const int b = blockIdx.y;
    const int f = xcd_remap(blockIdx.x, gridDim.x);
    const int Fb = a.F[b];
    if (f >= Fb) return;
    const Geo g = a.g;
    const int L = threadIdx.x;
    __shared__ double lds[WV_SLOTS];
    __shared__ double2 t2[64];  // W64^(p1 q2) at [q2][p1]
    const auto rS = buf_rsrc(a.S + ((int64_t)b * a.Fmax + f) * NB, NB * 4);
    const auto rC = buf_rsrc(a.winc, 4 * 64 * 16);
    const auto rT = buf_rsrc(a.c.tw, NFFT * 16);
    const auto rP = buf_rsrc(a.wt, 64 * 16);
    // ---- STFT input: z[L + 64 r] = x[2 (L + 64 r)] + i x[2 (L + 64 r) + 1], x = window * y_pad.
    // The periodic Hann at sample s is 1/2 - 1/2 c(s), c(s) = cos(2 pi (s - woff) / win); the lane's
    // samples step by 128 per register, so c follows the Chebyshev recurrence
    // c_{r+1} = 2 cos(theta) c_r - c_{r-1} (one fma per sample from two seeds per parity, a few
    // ulp over 16 steps, instead of 16 window-table loads).  Outside the support the sample is
    // exactly 0: the support-sized y range reads 0 there, or (reflected frames) a select.
    const double K = a.wrot;
    double2 v[16];
    const int r3 = L & 3, K2 = L >> 2;
    const int zb = wv_sig(L);                         // Z[L + 64 m]
    const int mb = wv_sig((64 - L) & 63) + (L == 0 ? 64 : 0);
    double zkr[8], zmr[8], z512r = 0.0, z512i = 0.0;
    t2[L] = buf_c64(rP, 16 * L, 0);  // first LDS use: ordered before the reads by the FFT's barriers
    if constexpr (!INIT) {
        const int N = g.hop * (Fb - 1);
        const int base = f * g.hop - NFFT / 2;
        float y0[16], y1[16];
        const bool interior = base + g.woff >= 0 && base + g.woff + g.win <= N;
        if (interior) {  // the support needs no reflection
            const auto rY = buf_rsrc(a.y + (int64_t)b * a.Nmax + base + g.woff, (unsigned)g.win * 4);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int s = 2 * (L + 64 * r) - g.woff;
                y0[r] = buf_f32(rY, s * 4);
                y1[r] = buf_f32(rY, (s + 1) * 4);
            }
        } else {
            const auto rY = buf_rsrc(a.y + (int64_t)b * a.Nmax, (unsigned)N * 4);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int s = 2 * (L + 64 * r);
                const bool i0 = s >= g.woff && s < g.woff + g.win, i1 = s + 1 >= g.woff && s + 1 < g.woff + g.win;
                y0[r] = i0 ? buf_f32(rY, reflect_idx(base + s, N) * 4) : 0.f;
                y1[r] = i1 ? buf_f32(rY, reflect_idx(base + s + 1, N) * 4) : 0.f;
            }
        }
        {
            const double2 s0 = buf_c64(rC, 16 * L, 0), s1 = buf_c64(rC, 16 * L, 1024);  // (c_0, c_1) per parity
            double a0 = s0.x, a1 = s0.y, b0 = s1.x, b1 = s1.y;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                v[r] = double2{fma(-0.5, a0, 0.5) * (double)y0[r], fma(-0.5, b0, 0.5) * (double)y1[r]};
                const double a2 = fma(K, a1, -a0), b2 = fma(K, b1, -b0);
                a0 = a1;
                a1 = a2;
                b0 = b1;
                b1 = b2;
            }
        }
        wave_fft1024<false>(v, lds, t2, rT, L);
        // ---- Z to LDS in natural (swizzled) order, real parts then imaginary parts; bin pairs
        // (k, 1024 - k), k = L + 64 m, m < 8, plus k = 512.  sig() only permutes bits 2-3 by bits 4-5,
        // so every address below is one per-lane base plus a multiple of 64 slots: Z[k] at zb + 64 m,
        // Z[1024 - k] at mb + 64 (15 - m) (for lane 0, m = 0 that is the spare slot 1024: Z[0] is taken
        // from its own Z[k] read, and the partner store that pair does not have lands there).  Every
        // LDS store is unconditional: a divergent store makes the compiler branch around the partner's
        // computation and spill.
        const int wb = wv_sig(16 * r3 + K2);              // this lane's output Z[256 q1 + 64 j + wb']
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q1 = 0; q1 < 4; ++q1) lds[wb + 256 * q1 + 64 * j] = v[4 * j + q1].x;
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            zkr[m] = lds[zb + 64 * m];
            zmr[m] = lds[mb + 64 * (15 - m)];
        }
        if (L == 0) zmr[0] = zkr[0];
        z512r = lds[512];  // sig(512) = 512
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q1 = 0; q1 < 4; ++q1) lds[wb + 256 * q1 + 64 * j] = v[4 * j + q1].y;
        __syncthreads();
        z512i = lds[512];
    }
    // One pair at a time (its imaginary parts, |S| and split twiddle read one pair ahead).  The
    // partner bin's pre-split value goes to lane (64 - L) & 63, register 15 - m (16 - m on lane 0),
    // i.e. to the slot of Z[1024 - k]: a slot only this lane reads (512 is read by one instruction
    // of all lanes and rewritten by lane 0 only), so it is stored in place with no barrier; its
    // real part at once, its imaginary part after the next barrier.  INIT: X from the phases.
    double vmy[8];
    double zki = 0.0, zmi = 0.0;
    if constexpr (!INIT) {
        zki = lds[zb];
        zmi = lds[mb + 64 * 15];
        if (L == 0) zmi = zki;
    }
    // INIT: the phases U of the lane's bins (k, 1024 - k per pair, then 512), all issued up front
    double uk[8], um[8], u512 = 0.0;
    auto phase_of = [&](int k) -> double {
        return a.phase_u ? a.phase_u[((int64_t)b * NB + k) * a.Fmax + f]
                         : hash_uniform(a.seed, ((unsigned long long)b * NB + k) * 1048576ull + f);
    };
    // exp(2 pi i U) |S| with .real at DC and Nyquist (gl_iter_kernel's init_bin)
    auto phase_bin = [&](int k, double sv, double u) -> double2 {
        double sn, cs;
        sincospi(2.0 * u, &sn, &cs);
        return double2{sv * cs, (k == 0 || k == NB - 1) ? 0.0 : sv * sn};
    };
    if constexpr (INIT) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            uk[m] = phase_of(L + 64 * m);
            um[m] = phase_of(NH - L - 64 * m);
        }
        u512 = phase_of(512);
    }
    double sa = buf_f32(rS, 4 * L), sb = buf_f32(rS, 4 * (NH - L));
    // split twiddles t[k] = W2048^(L + 64 m) = W2048^L x W32^m (compile-time W32^m)
    const double2 tL = buf_c64(rT, 16 * L, 0);
    double2 tk = tL;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        __builtin_amdgcn_sched_barrier(0);
        const int k = L + 64 * m;
        double zki_n = 0.0, zmi_n = 0.0, sa_n, sb_n = 0.0;
        double2 tk_n = double2{0.0, 0.0};
        if (m < 7) {
            if constexpr (!INIT) {
                zki_n = lds[zb + 64 * (m + 1)];
                zmi_n = lds[mb + 64 * (14 - m)];
            }
            sa_n = buf_f32s(rS, 4 * L, 256 * (m + 1));
            sb_n = buf_f32(rS, 4 * (NH - k - 64));
            tk_n = cmulf(tL, double2{kW32[m + 1][0], kW32[m + 1][1]});
        } else {
            sa_n = buf_f32s(rS, 0, 2048);  // k = 512
            tk_n = buf_c64(rT, 0, 8192);  // k = 512
        }
        double2 xk, xm;
        if constexpr (INIT) {
            xk = phase_bin(k, sa, uk[m]);
            xm = phase_bin(NH - k, sb, um[m]);
        } else {
            // 2E = Z[k] + conj Z[N-k], 2O = -i (Z[k] - conj Z[N-k]): X[k] = E + t O up to the factor 2
            const double2 E = double2{zkr[m] + zmr[m], zki - zmi};
            const double2 O = double2{zki + zmi, zmr[m] - zkr[m]};
            const double2 tO = cmulf(O, tk);
            xk = unit_phase(cadd(E, tO), sa);         // X[k]
            xm = unit_phase(cconj(csub(E, tO)), sb);  // X[1024 - k]
        }
        if ((L | m) == 0) {  // istft: .real of the Hermitian extension at DC and Nyquist
            xk.y = 0.0;
            xm.y = 0.0;
        }
        // the pair's two pre-splits share E, D and O: the partner's (conj t' = -t of bin 1024 - k)
        // is (E.x + O.y, O.x - E.y), E = X[k] + conj X[N-k], O = (X[k] - conj X[N-k]) conj(t)
        const double2 Ep = double2{xk.x + xm.x, xk.y - xm.y};
        const double2 Op = cmulcf(double2{xk.x - xm.x, xk.y + xm.y}, tk);
        v[m] = double2{Ep.x - Op.y, Ep.y + Op.x};
        const double2 vm = double2{Ep.x + Op.y, Op.x - Ep.y};
        lds[mb + 64 * (15 - m)] = vm.x;
        vmy[m] = vm.y;
        zki = zki_n;
        zmi = zmi_n;
        sa = sa_n;
        sb = sb_n;
        tk = tk_n;
    }
    __builtin_amdgcn_sched_barrier(0);
    double2 v512;
    {  // k = 512 pairs with itself: 2E = (2 Re Z, 0), 2O = (2 Im Z, 0)
        const double2 x = INIT ? phase_bin(512, sa, u512)
                               : unit_phase(double2{2.0 * z512r + 2.0 * z512i * tk.x, 2.0 * z512i * tk.y}, sa);
        v512 = inv_presplit2(x, x, tk);
    }
    lds[512] = v512.x;  // the same value from every lane
    __syncthreads();
#pragma unroll
    for (int R = 8; R < 16; ++R) v[R].x = lds[zb + 64 * R];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m)
        lds[mb + 64 * (15 - m)] = vmy[m];
    lds[512] = v512.y;
    __syncthreads();
#pragma unroll
    for (int R = 8; R < 16; ++R) v[R].y = lds[zb + 64 * R];
    __syncthreads();
    // ---- inverse FFT; z'[n] -> real samples 2n, 2n + 1; window the support and store float64
    // (the frame's store range is its support: stores outside it are dropped by the range check)
    wave_fft1024<true>(v, lds, t2, rT, L);
    // (samples 2 (16 r3 + K2) + 128 (j + 4 q1): the window by the same recurrence; each sample pair
    // is one 8-byte store (float32 pair; a wave's 64 pairs are 128 consecutive samples) into the
    // frame slot [fb, fb + winp), pairs outside the slot dropped by its range; the slot's one or two
    // samples outside the support are never read)
    const auto rO = buf_rsrc(static_cast<frame_t*>(a.next) + ((int64_t)b * a.Fmax + f) * g.winp, (unsigned)g.winp * 4);
    __builtin_amdgcn_sched_barrier(0);
    const double2 s0 = buf_c64(rC, 16 * L, 2048), s1 = buf_c64(rC, 16 * L, 3072);
    double a0 = s0.x, a1 = s0.y, b0 = s1.x, b1 = s1.y;
#pragma unroll
    for (int q1 = 0; q1 < 4; ++q1)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = 2 * (256 * q1 + 64 * j + 16 * r3 + K2);
            const double2 z = v[4 * j + q1];
            // (1/2 of the pre-split) x 1/NH: one exact power-of-two scale
            const float2 o2 = float2{(float)(fma(-0.5, a0, 0.5) * (z.x * (0.5 / NH))),
                                     (float)(fma(-0.5, b0, 0.5) * (z.y * (0.5 / NH)))};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o2), rO, (s - g.fb) * 4, 0, 0);
            const double a2 = fma(K, a1, -a0), b2 = fma(K, b1, -b0);
            a0 = a1;
            a1 = a2;
            b0 = b1;
            b1 = b2;
        }
}

// ---------------------------------------------------------------- persistent GL loop (small batches)
// Every GL iteration after the initial one, for all frames (<= 512 in all), in ONE launch: one
// workgroup per (sentence, frame) keeps its iteration-invariant operands (|S| row, window,
// twiddles, and the overlap-add geometry of its 2048 STFT input samples: contributor offsets and
// the window sum-square) in registers.  Frames are 8-byte granules {tag | float32 sample} (gran_t)
// in two ping-pong slots: iteration it reads slot it & 1 (tag it), writes slot (it + 1) & 1.
// Per iteration each thread re-reads the granules of its 8 input samples' <= 5 contributors until
// every tag is the iteration's (the neighbour wait and the overlap-add loads are one), then
// STFT -> S X/|X| -> iSTFT as gl_iter_kernel, and stores its frame's samples: no flag words, no
// per-frame publish.  Overwriting slot (it + 1) & 1 is safe because the contributor relation is
// symmetric (checked on the host for the geometry and frame count, gl_persistent_path): every
// reader of this frame's iteration it - 1 output is one of its own contributors, whose iteration
// it output this frame has read - so that reader has finished its iteration it - 1 gather.
// Placement: every workgroup publishes its XCD; frames map to XCDs in contiguous runs over the
// runtime placement.  A frame whose consumers (frames within 4; sentence edges excepted, where
// the STFT's reflection reaches further) share its XCD stores with workgroup scope (the line stays
// in that XCD's L2, where the consumers' sc1 loads read it); others write through (agent scope).
// A stale copy of a cross-XCD granule carries an old tag and is read again.  Waits are bounded.
struct PersArgs {
    IterArgs it;        // S, F, Fmax, B, geometry, constants (y / next / prev unused)
    gran_t* frames;     // [2][B][Fmax][winp]
    int64_t fstride;    // granules per slot
    int iters;          // iterations after the initial one
    unsigned* xtab;     // [B][Fmax] each workgroup's XCD, salted (zeroed by the initial iSTFT)
    unsigned salt;      // per launch (18 bits): tag(it) = salt << 14 | it
    long long tmo;      // wall_clock64 ticks per wait
    int* status;
    long long* prof;    // diagnostic (TTS_GL_PHASES): per-phase wall_clock64 ticks of frame prof_f, or null
    int prof_f;
    int nowait;         // measurement only (TTS_GL_NOWAIT=1): one gather sweep, tags unchecked (wrong results)
    int first_sleep;    // s_sleep(4) count before an iteration's first gather poll (TTS_GL_FIRST_SLEEP)
    int drop_f;         // fault injection (tests, TTS_GL_INJECT_DROP): sentence 0's frame drop_f stops
                        // after its first iteration without storing it (-1: none)
};
constexpr int GL_DMAX = 4;                            // overlap-add contributors lie within 4 frames
constexpr int GL_SLOTS = 2 * GL_DMAX + 1;              // gather buffer slots (frames f-4 .. f+4)
constexpr int GL_PAIRS = 9;                            // granule pairs per thread (<= 2304 per frame:
                                                       // 2216 at most for n_fft 2048 / win 1102 / hop 275)
// fill word of a fresh (or salt-wrapped) granule buffer, every dword: tag 1 = salt 0, never a live tag
constexpr unsigned GL_GRAN_FILL = 1u;

// TWO: the form for 257..512 frames, two workgroups per compute unit (one wave per SIMD each):
// at most 256 registers per lane (the FFT twiddles read pass by pass, fft1024_regs_gtw, instead of
// 48 VGPRs for the whole loop) and the spectrum X in the FFT buffer the forward transform does not
// end in, so the static LDS halves.  Same values, same operations: bitwise the one-per-CU form.
template <bool TWO>
__device__ __forceinline__ void gl_persistent_body(const PersArgs& p) {
    const IterArgs& a = p.it;
    const int b = blockIdx.y;
    const int Fb = a.F[b];
    if ((int)blockIdx.x >= Fb) return;  // (a speculative batch-1 run sizes the grid as an upper bound)
    const Geo g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ __align__(16) double2 buf0[NH];  // forward wave regions, then the spectrum X
    __shared__ __align__(16) double2 buf1[NH];  // Z, then the inverse wave regions
    __shared__ int sh[4];  // frame, local stores, abort
    auto fail = [&](int code) {
        fail_word(p.status, code);
        sh[2] = 1;
    };
    if (tid == 0) sh[2] = 0;
    // ---- placement: frames -> XCDs in contiguous runs over where the workgroups actually run
    const int xcc = xcc_id();
    unsigned* xt = p.xtab + (int64_t)b * a.Fmax;
    if (tid == 0) publish32_agent(xt + blockIdx.x, (p.salt << 8) | (unsigned)xcc);
    constexpr int PV = TWO ? 8 : 4;  // table entries per lane (Fb <= 64 PV)
    if (wave == 0) {
        unsigned v[PV];  // blocks PV lane .. PV lane + PV - 1
        // (a timed-out table still yields ranks below; the launch then fails with code 2)
        const bool ok = poll_until<0, 0>(
            [&] {
                bool ok = true;
#pragma unroll
                for (int i = 0; i < PV; ++i) {
                    const int k = lane * PV + i;
                    v[i] = k < Fb ? peek32(xt + k) : 0u;
                    ok = ok && (k >= Fb || (v[i] >> 8) == p.salt);
                }
                return ok;
            },
            p.tmo);
        int base = 0, cnt = 0, rank = 0;
        for (int x = 0; x < 8; ++x) {
            int c = 0, r = 0;
#pragma unroll
            for (int i = 0; i < PV; ++i) {
                const int k = lane * PV + i;
                const bool on = k < Fb && (int)(v[i] & 7) == x;
                c += __popcll(__ballot(on));
                r += __popcll(__ballot(on && k < (int)blockIdx.x));
            }
            if (x < xcc) base += c;
            if (x == xcc) { cnt = c; rank = r; }
        }
        if (lane == 0) {
            const int f = base + rank;
            sh[0] = f;
            sh[1] = f - 4 >= base && f + 4 < base + cnt && f >= 5 && f <= Fb - 6;
            if (!ok) fail(2);
        }
    }
    __syncthreads();
    if (sh[2]) return;
    const int f = sh[0];
    const bool local = sh[1];
    constexpr int PN = NFFT / GL_THREADS;
    // ---- iteration-invariant operands
    const spec_t* Sf = a.S + ((int64_t)b * a.Fmax + f) * NB;
    // the FFT twiddles in registers for the whole loop (one wave per SIMD: no occupancy to lose;
    // table reads where used cost latency on every pass here); TWO: read from the table
    std::conditional_t<TWO, TwMix, TwRegs> twf;
    twf.load(a.c.tw);  // (TWO: the table pointers are re-laundered every iteration: no hoisted pass reads)
    __shared__ __align__(16) double2 tw_pass[TWO ? TW_LDS : 1];
    if constexpr (TWO) TwMix::fill(tw_pass, a.c.tw);  // (ordered before its first use by the barriers below)
    // split twiddles (TWO: read from the table where used) and |S| of the thread's bins
    // k = bin2l(r) (layout B); thread 0 also holds the Nyquist bin's
    double2 tk[4];
    spec_t sk[4];  // (|S| in its float storage: widened where it is used)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        tk[r] = a.c.tw[bin2l(r)];
        sk[r] = Sf[bin2l(r)];
    }
    auto tkf = [&](int r) { return tk[r]; };
    const double2 tnyq = !TWO && tid == 0 ? a.c.tw[NH] : double2{0.0, 0.0};  // (TWO: from the table)
    const spec_t snyq = tid == 0 ? Sf[NH] : 0.f;
    // STFT input sample i of this thread: n = edge_sample(tid, i); its overlap-add contributors and
    // window sum-square, as ola_sample.  A contributor is an index into the gather buffer og: slot
    // s = fi - f + GL_DMAX holds frame fi's granule values (every contributor lies within GL_DMAX
    // frames, reflection included: checked here), index og_zero a 0.0 for absent ones.
    const int N = g.hop * (Fb - 1);
    extern __shared__ __align__(16) float og[];  // [GL_SLOTS][winp] + 2
    const int og_zero = GL_SLOTS * g.winp;
    __shared__ int rlo[GL_SLOTS], rhi[GL_SLOTS], rpre[GL_SLOTS + 1];
    if (tid < GL_SLOTS) {
        rlo[tid] = 0x7FFFFFFF;
        rhi[tid] = -1;
    }
    if (tid < 2) og[og_zero + tid] = 0.f;
    __syncthreads();
    double wi[PN];  // the window at this thread's samples: analysis (input) and synthesis (output) alike
    // contributor LDS indices, two 16-bit halves per register (og_zero < 65536: checked below)
    constexpr int OP = (OLA_MAX + 1) / 2;
    unsigned offp[PN][OP];
    float wssv[PN];
    if (og_zero > 0xFFFF) fail(6);
#pragma unroll
    for (int i = 0; i < PN; ++i) {
        const int n = edge_sample(tid, i);
        const bool sup = n >= g.woff && n < g.woff + g.win;
        wi[i] = sup ? a.c.win[n] : 0.0;
        const int q = reflect_idx(f * g.hop + n - NFFT / 2, N) + NFFT / 2;
        int ilo = q - g.woff - g.win + 1;
        ilo = ilo <= 0 ? 0 : (ilo + g.hop - 1) / g.hop;
        int ihi = (q - g.woff) / g.hop;
        if (ihi > Fb - 1) ihi = Fb - 1;
        const bool any = sup && q >= g.woff;
        float wss = 0.f;
#pragma unroll
        for (int k = 0; k < OP; ++k) offp[i][k] = 0u;
#pragma unroll
        for (int k = 0; k < OLA_MAX; ++k) {
            const int fi = ilo + k;
            const int o = q - fi * g.hop;
            const bool ok = any && fi <= ihi;
            const int sl = fi - f + GL_DMAX, gg = o - g.fb;
            if (ok && (sl < 0 || sl >= GL_SLOTS)) fail(4);  // (never: contributors are within GL_DMAX)
            const bool in = ok && sl >= 0 && sl < GL_SLOTS;
            offp[i][k >> 1] |= (unsigned)(in ? sl * g.winp + gg : og_zero) << (16 * (k & 1));
            if (in) {
                atomicMin(&rlo[sl], gg);
                atomicMax(&rhi[sl], gg);
            }
            wss = (float)((double)wss + (ok ? a.c.win2[o] : 0.0));
        }
        // (a sample whose sum-square is below FLT_MIN keeps its sum undivided: y / 1.0f == y)
        wssv[i] = wss > 1.17549435e-38f ? wss : 1.0f;
    }
    // The gather's loads: slot s needs granules [rlo, rhi] of frame f + s - GL_DMAX, read as
    // 16-byte-aligned pairs (winp is a multiple of 4: granule pairs start at even indices); pair u of
    // the workgroup goes to thread u % 256 (at most GL_PAIRS per thread).  gdst: LDS index | need
    // bits (bit 30: the pair's first granule is needed, bit 31: its second); pairs past the list
    // read out of range (zeros, to the zero word).
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int sl = 0; sl < GL_SLOTS; ++sl) {
            rpre[sl] = acc;
            acc += rhi[sl] >= 0 ? (rhi[sl] - (rlo[sl] & ~1)) / 2 + 1 : 0;
        }
        rpre[GL_SLOTS] = acc;
        if (acc > GL_PAIRS * GL_THREADS) fail(5);
    }
    __syncthreads();
    // (a listed pair needs at least one of its granules; its source offset is the LDS index
    // rebased to frame f - GL_DMAX: slot sl of the gather buffer mirrors frame f + sl - GL_DMAX)
    unsigned gdst[GL_PAIRS];
#pragma unroll
    for (int m = 0; m < GL_PAIRS; ++m) {
        const int u = tid + m * GL_THREADS;
        gdst[m] = (unsigned)og_zero;
        if (u < rpre[GL_SLOTS]) {
            int sl = 0;
            while (u >= rpre[sl + 1]) ++sl;
            const int g0 = (rlo[sl] & ~1) + 2 * (u - rpre[sl]);
            gdst[m] = (unsigned)(sl * g.winp + g0) | (g0 >= rlo[sl] ? 1u << 30 : 0u) | (g0 + 1 <= rhi[sl] ? 1u << 31 : 0u);
        }
    }
    const int gbase = (f - GL_DMAX) * g.winp * 8;
    auto goff = [&](int m) {
        return (gdst[m] >> 30) ? gbase + (int)(gdst[m] & 0x3FFFFFFFu) * 8 : OOB_OFF;
    };
    // byte offset of output sample i's granule in the frame slot (computed where stored); samples
    // outside the window support take an out-of-range offset (the buffer store drops them)
    // (TWO: computed where stored, from an opaque thread index: held, they would not fit)
    auto soff_of = [&](int t, int i) {
        const int e = edge_sample(t, i);
        return (unsigned)(e - g.woff) < (unsigned)g.win ? (e - g.fb) * 8 : OOB_OFF;
    };
    int soffv[TWO ? 1 : PN];
    if constexpr (!TWO) {
#pragma unroll
        for (int i = 0; i < PN; ++i) soffv[i] = soff_of(tid, i);
    }
    auto soff = [&](int i) { if constexpr (TWO) return soff_of(tid_opaque(), i); else return soffv[i]; };
    const bool timed = p.prof && f == p.prof_f && b == 0 && tid == 0;
    long long ph[6] = {0, 0, 0, 0, 0, 0};
    long long tp = timed ? (long long)wall_clock64() : 0;
#define GL_PHASE(k)                                      \
    if (timed) {                                         \
        const long long tn = (long long)wall_clock64(); \
        ph[k] += tn - tp;                                \
        tp = tn;                                         \
    }
    const unsigned tag0 = p.salt << 14;
    for (int it = 0; it < p.iters; ++it) {
        const gran_t* src = p.frames + (it & 1) * p.fstride + (int64_t)b * a.Fmax * g.winp;
        gran_t* dst = p.frames + ((it + 1) & 1) * p.fstride + ((int64_t)b * a.Fmax + f) * g.winp;
        const unsigned want = tag0 | (unsigned)it;
        if constexpr (TWO) {  // an opaque copy of the table pointer per iteration: loop-invariant table
            int z = 0;  // an opaque zero offset (the pointers keep their address spaces): table
            asm volatile("" : "+v"(z));  // reads hoisted out of the loop would not fit the registers
            twf.tw = (g_d*)a.c.tw + z;
            twf.pt = (l_d*)tw_pass + z;
        }
        // ---- gather: the workgroup's granule pairs (each thread <= GL_PAIRS 16-byte sc1 loads, all in
        // flight at once), re-read until every needed tag is this iteration's, then into LDS
        {
            const auto rG = buf_rsrc(src, (unsigned)(a.Fmax * g.winp * 8));
            u32x4 x[GL_PAIRS];
            first_poll_delay<4>(p.first_sleep);
            const bool ok = poll_until<0, GLP_SLEEP>(
                [&] {
#pragma unroll
                    for (int m = 0; m < GL_PAIRS; ++m)
                        x[m] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rG, goff(m), 0, SC1_VOLATILE));
                    bool ok = true;
#pragma unroll
                    for (int m = 0; m < GL_PAIRS; ++m)
                        ok = ok && (!(gdst[m] & (1u << 30)) || x[m].y == want) && (!(gdst[m] & (1u << 31)) || x[m].w == want);
                    return ok || p.nowait;  // (nowait: leaves after one sweep)
                },
                p.tmo);
            if (!ok && lane == 0) fail(1);
            // (unneeded granules of a pair land on LDS words no sum reads; out-of-range pairs write
            // zeros to the zero word)
#pragma unroll
            for (int m = 0; m < GL_PAIRS; ++m)
                *reinterpret_cast<float2*>(og + (gdst[m] & 0x3FFFFFFFu)) =
                    float2{__uint_as_float(x[m].x), __uint_as_float(x[m].z)};
        }
        __syncthreads();  // the gather buffer (or a timeout) before the sums and the FFT's LDS passes
        if (sh[2]) return;
        GL_PHASE(0)
        // ---- overlap-add sums (librosa istft: float64 contributions into a float32 signal, frame
        // order) straight into the forward FFT's layout-A registers
        double2 v[4];
#pragma unroll
        for (int i = 0; i < PN; ++i) {
            // (absent contributors read the zero word: adding +0.0 leaves the sum bitwise unchanged,
            // which is never -0.0)
            float y = 0.f;
#pragma unroll
            for (int k = 0; k < OLA_MAX; ++k) y = (float)((double)y + (double)og[(offp[i][k >> 1] >> (16 * (k & 1))) & 0xFFFFu]);
            const float yv = y / wssv[i];
            if (i & 1) v[i >> 1].y = wi[i] * (double)yv;
            else v[i >> 1].x = wi[i] * (double)yv;
        }
        GL_PHASE(1)
        fft2l_fwd(v, buf0, twf);
        GL_PHASE(2)
        double2 xnyq = double2{0.0, 0.0};
        spectrum2l(v, buf1, tkf, [&](int r) { return (double)sk[r]; }, TWO ? twf.tw_at(NH) : tnyq, (double)snyq, xnyq);
        presplit2l(v, buf0, tkf, xnyq);
        GL_PHASE(3)
        fft2l_inv(v, buf1, twf);
        GL_PHASE(4)
        if (b == 0 && f == p.drop_f) return;  // fault injection only: never stores iteration 1
        // ---- the frame's samples, tagged with the next iteration: XCD-local (workgroup-scope store,
        // the line stays in the XCD's L2) when every consumer shares this XCD, else written through
        const unsigned nt = tag0 | (unsigned)(it + 1);
        const auto rD = buf_rsrc(dst, (unsigned)g.winp * 8);
        // one 16-byte store per sample pair (2n, 2n + 1): two whole granules; a pair straddling an
        // end of the support also writes the slot's sample outside it (never read)
#pragma unroll
        for (int r = 0; r < PN / 2; ++r) {
            const u32x4 gv = u32x4{__float_as_uint((float)(wi[2 * r] * (v[r].x * (1.0 / NH)))), nt,
                                   __float_as_uint((float)(wi[2 * r + 1] * (v[r].y * (1.0 / NH)))), nt};
            const int e = edge_sample(TWO ? tid_opaque() : tid, 2 * r);
            const int off = e + 1 >= g.woff && e < g.woff + g.win ? (e - g.fb) * 8 : OOB_OFF;
            // plain (workgroup-scope) store: the line stays in this XCD's L2; sc1: written through
            if (local) __builtin_amdgcn_raw_buffer_store_b128(gv, rD, off, 0, 0);
            else __builtin_amdgcn_raw_buffer_store_b128(gv, rD, off, 0, 0x10);
        }
        GL_PHASE(5)
    }
#undef GL_PHASE
    if (timed)
        for (int k = 0; k < 6; ++k) p.prof[k] = ph[k];
}
__global__ __launch_bounds__(GL_THREADS) void gl_persistent_kernel(const PersArgs p) { gl_persistent_body<false>(p); }
__global__ __launch_bounds__(GL_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void gl_persistent2_kernel(
    const PersArgs p) {
    gl_persistent_body<true>(p);
}

// the initial iSTFT's granules (slot 0) as float32 frames for the fused loop, when the persistent
// launch could not be placed
__global__ void gl_gran_to_frames_kernel(const gran_t* in, float* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __uint_as_float((unsigned)in[i].v);
}

// ---------------------------------------------------------------- final OLA + inverse pre-emphasis
template <typename FT>
__global__ void gl_ola_kernel(const FinArgs a) {
    const int b = blockIdx.y;
    const int Fb = a.F[b];
    const int N = a.g.hop * (Fb - 1);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (a.host_status && p == 0 && b == 0) {  // the persistent loop's status, for the host's collect
        __hip_atomic_store(a.host_status, *a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.host_seq) release_word_system(a.host_seq, a.seq);
    }
    if (p >= N) return;
    // a persistent loop whose hand-off wait timed out left frames unwritten: never hand out a
    // plausible-looking waveform for it (the run's error status is raised when it is collected)
    const bool bad = a.status && *a.status != 0;
    // (contributor loads issued together when the geometry allows it: bitwise the same sum; the
    // window sum-square from the periodic table where no contributor is clipped, as ola_sample
    // would sum it, else summed here)
    const FT* fr = static_cast<const FT*>(a.frames) + (int64_t)b * a.Fmax * a.g.winp;
    const Geo& g = a.g;
    const int q = p + NFFT / 2;
    float yv;
    if ((g.win + g.hop - 1) / g.hop <= OLA_MAX && q >= g.woff) {
        const int u = q - g.woff;
        const int ihu = u / g.hop;
        int ilo = u - g.win + 1;
        const bool full = ilo >= 1 && ihu <= Fb - 1;
        ilo = ilo <= 0 ? 0 : (ilo + g.hop - 1) / g.hop;
        const int ihi = ihu > Fb - 1 ? Fb - 1 : ihu;
        double fv[OLA_MAX];
#pragma unroll
        for (int k = 0; k < OLA_MAX; ++k) {
            const int i = ilo + k;
            fv[k] = i <= ihi ? fval(fr[(int64_t)i * g.winp + (q - i * g.hop - g.fb)]) : 0.0;
        }
        float y = 0.f, wss = 0.f;
#pragma unroll
        for (int k = 0; k < OLA_MAX; ++k) y = (float)((double)y + fv[k]);
        if (full) {
            wss = a.wssp[u - ihu * g.hop];
        } else {
            for (int i = ilo; i <= ihi; ++i) wss = (float)((double)wss + a.c.win2[q - i * g.hop]);
        }
        yv = wss > 1.17549435e-38f ? y / wss : y;
    } else {
        yv = ola_sample(fr, q, Fb, g, a.c.win2);
    }
    a.y[(int64_t)b * a.Nmax + p] = bad ? __builtin_nanf("") : yv;
}

// gl_ola_kernel<frame_t> with OLA_R samples per thread (stride 256) and every contributor load
// (and window sum-square load) of the thread issued before the first sum: at one sample per
// thread a wave held ~1.3 KB of loads in flight, and the launch ran at ~2.9 TB/s (latency-bound by
// bytes in flight; configs[4]: 442 MB per launch).  Per sample the same loads and the same
// double-rounded sum order as gl_ola_kernel: bitwise equal.  Needs the unrolled geometry
// (ola_multi_ok).
constexpr int OLA_R = 4;
__device__ __forceinline__ int div_small(int n, int d, float rd) {  // floor(n / d), 0 <= n < 2^24
    int qt = (int)((float)n * rd);
    const int r = n - qt * d;
    qt += r >= d ? 1 : 0;
    qt -= r < 0 ? 1 : 0;
    return qt;
}
__global__ __launch_bounds__(256) void gl_ola_multi_kernel(const FinArgs a) {
    const int b = blockIdx.y;
    const int Fb = a.F[b];
    const Geo& g = a.g;
    const int N = g.hop * (Fb - 1);
    const int p0 = blockIdx.x * (256 * OLA_R) + threadIdx.x;
    if (a.host_status && p0 == 0 && b == 0) {
        __hip_atomic_store(a.host_status, *a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.host_seq) release_word_system(a.host_seq, a.seq);
    }
    if (p0 >= N) return;
    const bool bad = a.status && *a.status != 0;
    const float* fr = static_cast<const float*>(a.frames) + (int64_t)b * a.Fmax * g.winp;
    const float rhop = __builtin_amdgcn_rcpf((float)g.hop);
    const int step = g.winp - g.hop;  // frame i's element for sample q: i (winp - hop) + q - fb
    float fv[OLA_R][OLA_MAX], wv[OLA_R];
    int ilo[OLA_R], ihi[OLA_R];
#pragma unroll
    for (int j = 0; j < OLA_R; ++j) {
        const int q = p0 + 256 * j + NFFT / 2, u = q - g.woff;
        const int ihu = div_small(u, g.hop, rhop);
        int lo = u - g.win + 1;
        const bool full = lo >= 1 && ihu <= Fb - 1;
        lo = lo <= 0 ? 0 : div_small(lo + g.hop - 1, g.hop, rhop);
        const int hi = p0 + 256 * j < N ? min(ihu, Fb - 1) : -1;
        ilo[j] = lo;
        ihi[j] = hi;
        const int o = lo * step + q - g.fb;
#pragma unroll
        for (int k = 0; k < OLA_MAX; ++k) fv[j][k] = lo + k <= hi ? fr[o + k * step] : 0.f;
        wv[j] = full && hi >= 0 ? a.wssp[u - ihu * g.hop] : -1.f;  // -1: sum the window here
    }
#pragma unroll
    for (int j = 0; j < OLA_R; ++j) {
        const int p = p0 + 256 * j;
        if (p >= N) break;
        const int q = p + NFFT / 2;
        float y = 0.f;
#pragma unroll
        for (int k = 0; k < OLA_MAX; ++k) y = (float)((double)y + (double)fv[j][k]);
        float wss = wv[j];
        if (wss < 0.f) {
            wss = 0.f;
            for (int i = ilo[j]; i <= ihi[j]; ++i) wss = (float)((double)wss + a.c.win2[q - i * g.hop]);
        }
        const float yv = wss > 1.17549435e-38f ? y / wss : y;
        a.y[(int64_t)b * a.Nmax + p] = bad ? __builtin_nanf("") : yv;
    }
}
bool ola_multi_ok(const Geo& g, int64_t Nmax) {
    return (g.win + g.hop - 1) / g.hop <= OLA_MAX && g.woff <= NFFT / 2 && Nmax + NFFT < (1 << 24) &&
           (Nmax / g.hop + 2) * (int64_t)g.winp < (1ll << 31);  // (int frame offsets)
}
// the overlap-add of float32 frames (the fused / batched loops' slots) into the signal
void launch_ola_frames(const FinArgs& f, hipStream_t s) {
    static const bool single = env_is("TTS_GL_OLA_SINGLE", '1');  // measurement: one sample per thread
    if (!single && ola_multi_ok(f.g, f.Nmax))
        hipLaunchKernelGGL(gl_ola_multi_kernel, dim3((unsigned)((f.Nmax + 256 * OLA_R - 1) / (256 * OLA_R)), f.B),
                           dim3(256), 0, s, f);
    else
        hipLaunchKernelGGL(gl_ola_kernel<frame_t>, dim3((unsigned)((f.Nmax + 255) / 256), f.B), dim3(256), 0, s, f);
}

// y[n] = x[n] + c*y[n-1] in float64 (scipy.signal.lfilter([1], [1, -c], x), utils/audio.py:133-136).
// Chunk-parallel: workgroup (chunk i, sentence b) writes y[i*chunk, (i+1)*chunk) and starts its scan
// `look` samples earlier from y = 0: the state it misses is c^look * y, below 1e-22 of |y| (the host
// picks look from |c|; with look = 0 the one workgroup per sentence scans from sample 0, exactly the
// recurrence up to rounding order).  A tile of SCAN_THREADS*SCAN_PER samples: per-thread serial scan,
// then the (c^len, value) carries composed across lanes by shuffles and across waves through LDS.
__device__ __forceinline__ void scan_combine(double& A, double& Bv, double pa, double pb) {
    // (pa, pb) precedes (A, Bv): y_out = A (pa y_in + pb) + Bv
    Bv = fma(pb, A, Bv);
    A = pa * A;
}
__global__ __launch_bounds__(SCAN_THREADS) void preemph_scan_kernel(const float* y, int64_t Nmax, const int* F, int hop,
                                                                    double coef, int apply, int64_t chunk, int64_t look,
                                                                    double* wav) {
    const int b = blockIdx.y;
    const int64_t N = (int64_t)hop * (F[b] - 1);
    const int64_t o0 = (int64_t)blockIdx.x * chunk;
    if (o0 >= N) return;
    const int64_t o1 = o0 + chunk < N ? o0 + chunk : N;
    const float* x = y + (int64_t)b * Nmax;
    double* o = wav + (int64_t)b * Nmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!apply) {
        for (int64_t i = o0 + tid; i < o1; i += SCAN_THREADS) o[i] = (double)x[i];
        return;
    }
    constexpr int TILE = SCAN_THREADS * SCAN_PER, NW = SCAN_THREADS / 64;
    __shared__ double wa[NW], wb[NW];
    double cpow[SCAN_PER + 1];
    cpow[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= SCAN_PER; ++k) cpow[k] = cpow[k - 1] * coef;
    const int64_t s0 = o0 - look > 0 ? ((o0 - look) & ~(int64_t)7) : 0;
    double carry = 0.0;  // y at the end of the previous tile
    for (int64_t t0 = s0; t0 < o1; t0 += TILE) {
        const int64_t base = t0 + (int64_t)tid * SCAN_PER;
        double v = 0.0, loc[SCAN_PER];
#pragma unroll
        for (int k = 0; k < SCAN_PER; ++k) {
            v = (base + k < o1 ? (double)x[base + k] : 0.0) + coef * v;
            loc[k] = v;
        }
        // inclusive composition over the lanes of this wave
        double A = cpow[SCAN_PER], Bv = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double pa = __shfl_up(A, off, 64), pb = __shfl_up(Bv, off, 64);
            if (lane >= off) scan_combine(A, Bv, pa, pb);
        }
        if (lane == 63) { wa[wave] = A; wb[wave] = Bv; }
        __syncthreads();
        // every wave composes the waves' totals itself (NW lanes), then takes its carry-in
        double WA = lane < NW ? wa[lane] : 1.0, WB = lane < NW ? wb[lane] : 0.0;
#pragma unroll
        for (int off = 1; off < NW; off <<= 1) {
            const double qa = __shfl_up(WA, off, 64), qb = __shfl_up(WB, off, 64);
            if (lane >= off) scan_combine(WA, WB, qa, qb);
        }
        const double win_in = wave == 0 ? carry : __shfl(WA, wave - 1, 64) * carry + __shfl(WB, wave - 1, 64);
        const double tile_end = __shfl(WA, NW - 1, 64) * carry + __shfl(WB, NW - 1, 64);
        // y entering this thread: compose the lanes before it (exclusive) with the wave's carry-in
        const double pa = __shfl_up(A, 1, 64), pb = __shfl_up(Bv, 1, 64);
        const double cin = lane == 0 ? win_in : pa * win_in + pb;
#pragma unroll
        for (int k = 0; k < SCAN_PER; ++k) {
            const int64_t i = base + k;
            if (i >= o0 && i < o1) o[i] = loc[k] + cpow[k + 1] * cin;
        }
        carry = tile_end;
        __syncthreads();  // wa / wb are rewritten by the next tile
    }
}

// one iteration's STFT -> phase -> iSTFT launch in the form a run takes (gl_run_dev's graphs, tts_gl_profile)
void launch_iteration(bool fused, bool wave, const IterArgs& a, hipStream_t s) {
    const dim3 grid(a.Fmax, a.B), block(GL_THREADS);
    if (fused) hipLaunchKernelGGL((gl_iter_kernel<false, true, frame_t>), grid, block, 0, s, a);
    else if (wave) hipLaunchKernelGGL(gl_iter_wave_kernel<false>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((gl_iter_kernel<false, false, frame_t>), grid, block, 0, s, a);
}

// small batches fuse the overlap-add into the iteration launch; at most 256 frames in all run the
// whole loop as one persistent launch (host values only)
bool gl_fused_path(const tts_gl* g, int B, int Fmax) {
    return ((int64_t)B * Fmax <= 1024 || env_is("TTS_GL_FUSED", '1')) && (g->g.win + g->g.hop - 1) / g->g.hop <= OLA_MAX;
}
// The persistent loop overwrites a frame's ping-pong slot once its own contributors have moved on:
// safe when every reader of a frame is one of its contributors.  Frame f reads the signal at the
// reflected positions R(W_f), W_f = [f hop - win/2, f hop + win/2) (centred STFT frames), and its
// contributors are the frames fi whose windows W_fi hold one of them.  Between two frames whose
// windows lie inside [0, N) "f reads fi" <=> W_f n W_fi != {} is symmetric.  A frame whose window
// reaches a sentence edge reads R(W_f), which is not W_f n [0, N): position -win/2 reflects to
// win/2, one past W_0, and N + win/2 - 1 to N - win/2 - 1, one before W_(F-1); whether a frame that
// W_f itself does not meet contributes there depends on the geometry (at win = 4 hop, win even,
// frame 0 reads frame 4 and frame F - 1 reads frame F - 5 from six frames up, and neither is read
// back; at 1102 / 275 the same positions fall to frames the window meets anyway).  So every frame
// count is checked by brute force (host copy of the kernels' index maps).
int reflect_host(int p, int N) {
    if ((unsigned)p < (unsigned)N) return p;
    if (N == 1) return 0;
    const int period = 2 * (N - 1);
    int pp = p % period;
    if (pp < 0) pp += period;
    return pp < N ? pp : period - pp;
}
// The overlap-add contributors of frame f of an F-frame sentence: fn(q, ilo, fi) for every sample
// of the frame's window (q its reflected, untrimmed position) and every frame fi in ola_sample's
// range [ilo, ihi] for it.  Stops, and returns false, when fn does.
template <class Fn>
bool for_contributors(const Geo& g, int f, int F, Fn fn) {
    const int N = g.hop * (F - 1);
    for (int n = g.woff; n < g.woff + g.win; ++n) {
        const int q = reflect_host(f * g.hop + n - NFFT / 2, N) + NFFT / 2;
        if (q < g.woff) continue;
        int ilo = q - g.woff - g.win + 1;
        ilo = ilo <= 0 ? 0 : (ilo + g.hop - 1) / g.hop;
        const int ihi = std::min((q - g.woff) / g.hop, F - 1);
        for (int fi = ilo; fi <= ihi; ++fi)
            if (!fn(q, ilo, fi)) return false;
    }
    return true;
}
// Rows of the relation are built for the frames near either end only: the frames whose window reaches
// an edge (at most win / (2 hop) + 1 per end) and the 2 OLA_MAX frames next to them, all frames of a
// short sentence.  Any other pair of frames is symmetric by the argument above, and a frame outside
// the rows reads nothing beyond OLA_MAX frames from itself, so an edge frame that reads it is not read back.
bool contrib_symmetric(const Geo& g, int F) {
    const int N = g.hop * (F - 1);
    auto edge = [&](int f) {
        return f * g.hop + g.woff - NFFT / 2 < 0 || f * g.hop + g.woff + g.win - 1 - NFFT / 2 >= N;
    };
    const int K = g.win / (2 * g.hop) + 2 + 2 * OLA_MAX;  // rows per end
    std::vector<int> rows;
    for (int f = 0; f < F; ++f)
        if (f < K || f >= F - K) rows.push_back(f);
    std::vector<int> row_of(F, -1);
    for (size_t r = 0; r < rows.size(); ++r) row_of[rows[r]] = (int)r;
    std::vector<char> c(rows.size() * (size_t)F, 0);
    for (size_t r = 0; r < rows.size(); ++r)
        for_contributors(g, rows[r], F, [&](int, int, int fi) { return c[r * F + fi] = 1; });
    for (size_t r = 0; r < rows.size(); ++r)
        for (int fi = 0; fi < F; ++fi) {
            const char reads = c[r * F + fi];
            if (row_of[fi] >= 0) {
                if (reads != c[(size_t)row_of[fi] * F + rows[r]]) return false;
            } else if (reads && edge(rows[r])) {
                return false;
            }
        }
    return true;
}
// The persistent loop's gather layout for a sentence of F frames (gl_persistent_kernel): every
// overlap-add contributor within GL_DMAX frames and at most GL_PAIRS granule pairs per thread.  Only
// frames whose STFT window reaches a sentence edge (reflection) differ from the interior ones: those
// and one interior frame are checked, restating the kernel's index arithmetic.
bool gather_fits(const Geo& g, int F) {
    const int N = g.hop * (F - 1);
    auto frame_ok = [&](int f) {
        int lo[GL_SLOTS], hi[GL_SLOTS];
        for (int k = 0; k < GL_SLOTS; ++k) {
            lo[k] = 1 << 30;
            hi[k] = -1;
        }
        const bool near = for_contributors(g, f, F, [&](int q, int ilo, int fi) {
            const int sl = fi - f + GL_DMAX;
            if (sl < 0 || sl >= GL_SLOTS || fi - ilo >= OLA_MAX) return false;
            lo[sl] = std::min(lo[sl], q - fi * g.hop - g.fb);
            hi[sl] = std::max(hi[sl], q - fi * g.hop - g.fb);
            return true;
        });
        if (!near) return false;
        int pairs = 0;
        for (int k = 0; k < GL_SLOTS; ++k)
            if (hi[k] >= 0) pairs += (hi[k] - (lo[k] & ~1)) / 2 + 1;
        return pairs <= GL_PAIRS * GL_THREADS;
    };
    bool interior_done = false;
    for (int f = 0; f < F; ++f) {
        const bool edge = f * g.hop + g.woff - NFFT / 2 < 0 || f * g.hop + g.woff + g.win - 1 - NFFT / 2 >= N;
        if (!edge && interior_done) continue;
        if (!frame_ok(f)) return false;
        if (!edge) interior_done = true;
    }
    return (g.winp % 2) == 0;
}

// ---- gl_run_dev: workspace, path, frame counts, phases, the three loops, the final overlap-add ----

// What the stages of one gl_run_dev share; the driver builds it on its stack.
struct RunCtx {
    int mode;
    const float* spec;
    const int32_t* F;  // host frame counts (upper bounds when F_bound)
    const int* F_dev;  // the counts on the device, or null
    bool F_bound;
    int B, Fmax, iters;
    const double* phase_u;  // the caller's initial phases, then the numpy-stream draw's, or null
    uint64_t seed;
    double* wav;
    hipStream_t cs, s;  // the caller's stream; the one the run is enqueued on
    int64_t Nmax;
    size_t fstride;    // elements of one of the two frame slots
    int frames_total;
    bool fused, persistent;  // the path chosen from host values
    bool persistent_ran;     // ... and whether the persistent launch was placed
    bool timed;  // loop timers and the completion event (outside pipeline mode)
    const int* Fd;  // the frame counts the launches read: F_dev, or the handle's own array
    IterArgs ia;
    FinArgs fa;
};

// frame slot i of the two ping-pong slots of the fused / batched loops
frame_t* frame_slot(const tts_gl* g, const RunCtx& c, int i) { return g->frames.p + (i & 1) * c.fstride; }

// workspace (grow only; graphs bake the buffer addresses and are dropped when they move), then the
// hand-over from the caller's stream
tts_status reserve_workspace(tts_gl* g, const RunCtx& c) {
    const size_t BF = (size_t)c.B * c.Fmax;
    bool moved = false;
    // the workspace may move below: nothing of this handle may still be in flight (a pipeline
    // run's stream has been synchronised by its caller before the next run)
    if (!g->pipeline) TTS_HIP(hipStreamSynchronize(c.s));
    TTS_TRY(g->S.reserve(BF * NB, &moved));
    TTS_TRY(g->frames.reserve(2 * BF * g->g.winp, &moved));
    TTS_TRY(g->y.reserve((size_t)c.B * c.Nmax, &moved));
    TTS_TRY(g->F.reserve(c.B, &moved));
    if (moved) {
        for (auto& kv : g->graphs) (void)hipGraphExecDestroy(kv.second);
        g->graphs.clear();
    }
    if (c.s != c.cs) {
        TTS_HIP(hipEventRecord(g->ev_in, c.cs));
        TTS_HIP(hipStreamWaitEvent(c.s, g->ev_in, 0));
    }
    return TTS_OK;
}

// the handle's own frame-count array from the device counts (a speculative run's host F is only an
// upper bound: tts_synth_run) or from the host's
tts_status stage_counts(tts_gl* g, const RunCtx& c) {
    if (c.F_bound) TTS_HIP(hipMemcpyAsync(g->F.p, c.F_dev, c.B * sizeof(int), hipMemcpyDeviceToDevice, c.s));
    else TTS_HIP(hipMemcpyAsync(g->F.p, c.F, c.B * sizeof(int), hipMemcpyHostToDevice, c.s));
    return TTS_OK;
}

// the reference's np.random.rand draws, continued on the device from numpy's state
// (tts_gl_set_phase_state): one [1025][F_b] draw per sentence in batch order
tts_status draw_phases(tts_gl* g, RunCtx& c) {
    if (c.phase_u || !g->mt_armed) return TTS_OK;
    const size_t need = (size_t)c.B * NB * c.Fmax;
    if (need > g->mt_phase.cap && g->mt_stream) TTS_HIP(hipStreamSynchronize(g->mt_stream));  // an earlier run may still read it
    TTS_TRY(g->mt_phase.reserve(need));
    TTS_TRY(mt_draw(g, c.Fd, c.B, c.Fmax, g->mt_phase.p, c.s));
    c.phase_u = g->mt_phase.p;
    return TTS_OK;
}

tts_status launch_magnitude(tts_gl* g, const RunCtx& c) {
    MagArgs ma{};
    ma.mode = c.mode;
    ma.spec = c.spec;
    ma.n_in = c.mode == TTS_GL_FROM_MEL ? g->cfg.num_mels : NB;
    ma.Fmax = c.Fmax;
    ma.F = c.Fd;
    ma.pinv = g->pinv;
    ma.S = g->S.p;
    ma.min_db = g->cfg.min_level_db;
    ma.ref_db = g->cfg.ref_level_db;
    ma.power = g->cfg.power;
    ma.max_norm = g->cfg.max_norm;
    ma.signal_norm = g->cfg.signal_norm;
    ma.symmetric = g->cfg.symmetric_norm;
    ma.clip = g->cfg.clip_norm;
    if (c.mode == TTS_GL_FROM_LINEAR)
        hipLaunchKernelGGL(gl_linear_magnitude_kernel,
                           dim3((unsigned)(((int64_t)c.Fmax * NB + 256 * LIN_PER - 1) / (256 * LIN_PER)), c.B), dim3(256), 0,
                           c.s, ma);
    else
        hipLaunchKernelGGL(gl_magnitude_kernel, dim3((NB + MAG_KT - 1) / MAG_KT, (c.Fmax + MAG_FT - 1) / MAG_FT, c.B),
                           dim3(256), 0, c.s, ma);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

// The initial iSTFT into slot 0 (the persistent loop: into tagged granules, with its tag words and
// status word cleared), the loop's start timer, and the arguments every later launch starts from.
tts_status launch_init(tts_gl* g, RunCtx& c) {
    hipStream_t s = c.s;
    // the persistent loop reads and writes two slots of tagged granules (gl_persistent_kernel);
    // the other loops two slots of float32 frames (TTS_GL_FUSED=1 forces the fused form at any
    // batch: measurement knob)
    if (c.persistent) {
        bool fresh = false;
        TTS_TRY(g->pgr.reserve(2 * c.fstride, &fresh));
        // fresh memory may hold a freed handle's granules, and every handle's salts start at 1: a
        // stale granule there can carry a tag this handle is about to wait for.  Filled with a word
        // that is no live tag and not 0 (0 marks an absent contributor: gl_persistent_kernel)
        if (fresh) TTS_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g->pgr.p), GL_GRAN_FILL, g->pgr.cap * 2, s));
        // the initial iSTFT tags its granules with the launch's salt
        g->salt = (g->salt + 1) & 0x3FFFF;
        if (g->salt == 0) {
            // wrapped: a granule of the launch 2^18 back could carry a current tag
            g->salt = 1;
            TTS_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g->pgr.p), GL_GRAN_FILL, g->pgr.cap * 2, s));
        }
    }
    IterArgs& ia = c.ia;
    ia.S = g->S.p;
    ia.F = c.Fd;
    ia.Fmax = c.Fmax;
    ia.B = c.B;
    ia.g = g->g;
    ia.c = GLConst{g->win, g->win2, g->tw};
    ia.phase_u = c.phase_u;
    ia.seed = c.seed;
    ia.y = g->y.p;
    ia.Nmax = c.Nmax;
    ia.next = c.persistent ? static_cast<void*>(g->pgr.p) : frame_slot(g, c, 0);
    ia.wt = g->wt;
    ia.winc = g->winc;
    ia.wrot = g->wrot;
    ia.gtag = g->salt << 14;
    if (c.persistent) {
        TTS_TRY(g->flags.reserve((size_t)c.B * c.Fmax));
        // table entries are salted per launch, and a new handle can get a freed one's words: the
        // initial iSTFT launch zeroes them and the status word
        ia.zero_flags = g->flags.p;
        ia.zero_status = g->pstatus;
    }
    const dim3 grid(c.Fmax, c.B), block(GL_THREADS);
    static const bool wave_init = !env_is("TTS_GL_WAVE_INIT", '0');  // measurement: 0 keeps the block-kernel init
    if (c.persistent) hipLaunchKernelGGL((gl_iter_kernel<true, false, gran_t>), grid, block, 0, s, ia);
    else if (!c.fused && g->wave && wave_init)  // the batched loop's own layout for its first launch
        hipLaunchKernelGGL(gl_iter_wave_kernel<true>, grid, dim3(64), 0, s, ia);
    else hipLaunchKernelGGL((gl_iter_kernel<true, false, frame_t>), grid, block, 0, s, ia);
    ia.zero_flags = nullptr;
    ia.zero_status = nullptr;
    TTS_HIP(hipGetLastError());
    // loop timers and the completion event outside pipeline mode only (each event marker holds the
    // GPU ~5.8 us between the kernels around it); a pipeline run's status travels by sequence word
    if (c.timed) TTS_HIP(hipEventRecord(g->ev_t0, s));
    FinArgs& fa = c.fa;
    fa.F = c.Fd;
    fa.Fmax = c.Fmax;
    fa.B = c.B;
    fa.g = g->g;
    fa.c = ia.c;
    fa.y = g->y.p;
    fa.Nmax = c.Nmax;
    fa.wssp = g->wssp;
    return TTS_OK;
}

// diagnostic (TTS_GL_PHASES): the phase ticks of one frame of the persistent loop, to stderr
tts_status report_gl_phases(long long* prof, int frame, int iters, hipStream_t s) {
    long long h[6];
    TTS_HIP(hipMemcpyAsync(h, prof, sizeof(h), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipStreamSynchronize(s));
    TTS_HIP(hipFree(prof));
    int rate_khz = 100000, dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev);
    static const char* names[6] = {"gather", "ola_sums", "fwd_fft", "spectrum", "inv_fft", "store"};
    fprintf(stderr, "TTS_GL_PHASES frame %d, us per iteration:", frame);
    for (int k = 0; k < 6; ++k) fprintf(stderr, " %s %.3f", names[k], h[k] * 1e3 / rate_khz / iters);
    fprintf(stderr, "\n");
    return TTS_OK;
}

// The whole loop as one launch.  Every workgroup waits on its neighbours inside it: co-residency
// guaranteed, or nothing runs (persistent_ran stays false), slot 0 of the granule buffer is handed
// over as float32 frames and the graph-replayed loop takes the iterations (bitwise the same waveform).
tts_status run_persistent(tts_gl* g, RunCtx& c) {
    hipStream_t s = c.s;
    PersArgs pa{};
    pa.it = c.ia;
    pa.frames = g->pgr.p;
    pa.fstride = (int64_t)c.fstride;
    pa.iters = c.iters;
    pa.xtab = g->flags.p;
    pa.salt = g->salt;
    pa.tmo = g->tmo;
    pa.status = g->pstatus;
    pa.drop_f = -1;
    if (const char* inj = getenv("TTS_GL_INJECT_DROP"); inj && inj[0]) pa.drop_f = atoi(inj);
    static const bool gl_nowait = env_is("TTS_GL_NOWAIT", '1');
    pa.nowait = gl_nowait;
    // round 6: -19 us per configs[1] sentence (tools/cases_sleep.txt)
    static const int gl_first_sleep = env_int("TTS_GL_FIRST_SLEEP", 4);
    pa.first_sleep = gl_first_sleep;
    long long* prof = nullptr;
    const char* phases = getenv("TTS_GL_PHASES");
    if (phases && phases[0]) {  // diagnostic: phase ticks of frame TTS_GL_PHASES (stderr)
        TTS_HIP(hipMalloc(&prof, 6 * sizeof(long long)));
        TTS_HIP(hipMemsetAsync(prof, 0, 6 * sizeof(long long), s));
        pa.prof = prof;
        pa.prof_f = std::min(atoi(phases), c.frames_total - 1);
    }
    void* kargs[] = {&pa};
    // dynamic LDS: the gather buffer, GL_SLOTS frame slots + the zero word
    const size_t og_bytes = ((size_t)GL_SLOTS * g->g.winp + 2) * sizeof(float);
    // up to 256 workgroups: one per compute unit; up to 512: two per compute unit (gl_persistent2_kernel)
    const dim3 grid(c.Fmax, c.B), block(GL_THREADS);
    const bool two = (long long)grid.x * grid.y > 256;
    const void* pfn = two ? reinterpret_cast<const void*>(&gl_persistent2_kernel)
                          : reinterpret_cast<const void*>(&gl_persistent_kernel);
    static const hipError_t attr = [] {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gl_persistent_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gl_persistent2_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        return e;
    }();
    TTS_HIP(attr);
    TTS_CHECK(og_bytes <= 96 * 1024, TTS_ERR_INVALID, "persistent Griffin-Lim: window too long for the gather buffer");
    TTS_HIP(launch_persistent(pfn, grid, block, kargs, og_bytes, s, &c.persistent_ran));
    if (!c.persistent_ran) {
        // the initial iSTFT wrote slot 0 of the granule buffer: hand it to the fused loop
        hipLaunchKernelGGL(gl_gran_to_frames_kernel, dim3((unsigned)((c.fstride + 255) / 256)), dim3(256), 0, s,
                           g->pgr.p, g->frames.p, (int64_t)c.fstride);
        TTS_HIP(hipGetLastError());
        if (prof) {
            TTS_HIP(hipStreamSynchronize(s));
            TTS_HIP(hipFree(prof));
        }
    } else if (prof) {
        TTS_TRY(report_gl_phases(prof, pa.prof_f, c.iters, s));
    }
    return TTS_OK;
}

// The iterations as one graph per (B, Fmax, iters), captured on first use.  One iteration =
// overlap-add of the previous frames into the float32 signal (every sample once) + one workgroup
// per frame for STFT -> phase -> iSTFT of that signal; the fused form gathers inside that launch.
tts_status run_graph_loop(tts_gl* g, const RunCtx& c) {
    hipStream_t s = c.s;
    GraphKey key{c.B, c.Fmax, c.iters};
    auto it = g->graphs.find(key);
    if (it == g->graphs.end()) {
        hipGraph_t graph = nullptr;
        TTS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < c.iters; ++i) {
            IterArgs a = c.ia;
            a.phase_u = nullptr;
            a.next = frame_slot(g, c, i + 1);
            if (c.fused) {
                a.prev = frame_slot(g, c, i);
            } else {
                FinArgs o = c.fa;
                o.frames = frame_slot(g, c, i);
                launch_ola_frames(o, s);
            }
            launch_iteration(c.fused, g->wave, a, s);
        }
        hipError_t ce = hipGetLastError();
        hipError_t ee = hipStreamEndCapture(s, &graph);
        TTS_HIP(ce);
        TTS_HIP(ee);
        hipGraphExec_t exec = nullptr;
        TTS_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        TTS_HIP(hipGraphDestroy(graph));
        it = g->graphs.emplace(key, exec).first;
    }
    TTS_HIP(hipGraphLaunch(it->second, s));
    return TTS_OK;
}

// The loop's end timer, the final overlap-add (after a persistent loop: with its status word and,
// in pipeline mode, the sequence word the host waits for) and the de-emphasis scan into wav.
tts_status finish(tts_gl* g, RunCtx& c) {
    hipStream_t s = c.s;
    FinArgs& fa = c.fa;
    if (c.timed) TTS_HIP(hipEventRecord(g->ev_t1, s));
    fa.frames = c.persistent_ran ? static_cast<void*>(g->pgr.p + (size_t)(c.iters & 1) * c.fstride)
                                 : frame_slot(g, c, c.iters);
    fa.status = c.persistent_ran ? g->pstatus : nullptr;
    fa.host_status = c.persistent_ran ? g->host_status : nullptr;  // (no read-back copy launch)
    if (c.persistent_ran && !c.timed) {
        fa.host_seq = g->host_status + 1;
        fa.seq = ++g->seq;
        g->seq_stream = s;
    }
    if (c.persistent_ran)
        hipLaunchKernelGGL(gl_ola_kernel<gran_t>, dim3((c.Nmax + 255) / 256, c.B), dim3(256), 0, s, fa);
    else launch_ola_frames(fa, s);
    fa.status = nullptr;
    fa.host_status = nullptr;
    fa.host_seq = nullptr;
    TTS_HIP(hipGetLastError());
    // de-emphasis chunks: each starts `look` samples early, |c|^look <= 1e-22; one chunk per
    // sentence (look 0) when that does not fit one scan tile
    const double cf = g->cfg.preemphasis, ac = std::fabs(cf);
    int64_t chunk = SCAN_CHUNK, look = 0;
    if (ac > 0.0) {
        const double need = ac < 1.0 ? std::ceil(std::log(1e-22) / std::log(ac)) : 1e30;
        if (need <= (double)(SCAN_THREADS * SCAN_PER - SCAN_CHUNK - 8)) look = (int64_t)need;
        else chunk = c.Nmax;
    }
    const dim3 sgrid((unsigned)((c.Nmax + chunk - 1) / chunk), c.B);
    hipLaunchKernelGGL(preemph_scan_kernel, sgrid, dim3(SCAN_THREADS), 0, s, g->y.p, c.Nmax, c.Fd, g->g.hop, cf,
                       cf != 0.0 ? 1 : 0, chunk, look, c.wav);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

// what tts_gl_last_path / tts_gl_last_timing / tts_gl_profile report, the completion event, and
// (outside pipeline mode) the wait for the run
tts_status record_last(tts_gl* g, const RunCtx& c) {
    g->last_persistent = c.persistent_ran;
    g->last_path = c.persistent_ran ? TTS_GL_PATH_PERSISTENT : c.fused ? TTS_GL_PATH_FUSED : TTS_GL_PATH_UNFUSED;
    g->last_launches = c.persistent_ran ? 1 : (c.fused ? 1 : 2) * c.iters;
    if (c.timed) {
        TTS_HIP(hipEventRecord(g->ev_done, c.s));
        if (c.s != c.cs) TTS_HIP(hipStreamWaitEvent(c.cs, g->ev_done, 0));
    } else {
        g->last_ms = 0.f;  // (pipeline mode: not timed)
    }
    g->last_timed = c.timed;
    g->pending = true;
    if (!g->pipeline) TTS_TRY(gl_collect(g));
    g->last_fused = c.fused;
    g->have_last = true;
    g->last_iter = c.ia;
    g->last_fin = c.fa;
    g->last_fstride = c.fstride;
    return TTS_OK;
}

}  // namespace

namespace tts {

bool gl_persistent_path(tts_gl* g, int B, int Fmax, int frames_total, int iters) {
    // (tags hold the iteration in 14 bits below the salt)
    if (!(gl_fused_path(g, B, Fmax) && iters > 0 && iters < (1 << 14) && frames_total <= 512 && g->tmo > 0 &&
          !env_is("TTS_RESIDENT", '0')))
        return false;
    // every frame count the run may have (a speculative run knows only the upper bound Fmax): a
    // geometry or length the loop is not safe for takes the fused loop instead
    if ((int)g->gather_fit.size() <= Fmax) g->gather_fit.resize(Fmax + 1, -1);
    for (int F = 2; F <= Fmax; ++F) {
        if (g->gather_fit[F] < 0) g->gather_fit[F] = contrib_symmetric(g->g, F) && gather_fits(g->g, F) ? 1 : 0;
        if (!g->gather_fit[F]) return false;
    }
    return true;
}

tts_status gl_collect(tts_gl* g) {
    if (!g->pending) return TTS_OK;
    g->pending = false;
    if (g->last_timed) {
        TTS_HIP(hipEventSynchronize(g->ev_done));
        TTS_HIP(hipEventElapsedTime(&g->last_ms, g->ev_t0, g->ev_t1));
    } else if (g->last_persistent) {
        // pipeline mode: no event markers; the overlap-add launch set the status, then the sequence
        TTS_HIP(spin_word(g->host_status + 1, g->seq, g->seq_stream));
    }
    if (g->last_persistent)
        // (the kernel's code: 1 a gather wait, 2 the placement table, 4 / 5 / 6 a layout the host should have refused)
        TTS_CHECK(g->host_status[0] == 0, TTS_ERR_HIP,
                  "persistent Griffin-Lim: a hand-off wait timed out (internal error, code " +
                      std::to_string(g->host_status[0]) + ")");
    return TTS_OK;
}

// tts_gl_run, optionally with the frame counts also on the device (F_dev, the same values as F:
// tts_synth_run passes the decoder's step counts at r = 1): the persistent loop's launches then
// read them there and the upload is skipped (the graph-replayed fallbacks still upload into the
// handle's own array, which their graphs bake in).  F_bound: F holds only upper bounds of the
// device counts (a run enqueued before the decoder's step counts reach the host, same stream):
// the fallbacks then copy F_dev into the handle's array on the device.
tts_status gl_run_dev(tts_gl* g, int mode, const float* spec, const int32_t* F, const int* F_dev, int B, int Fmax,
                      const double* phase_u, uint64_t seed, int iters, double* wav, hipStream_t stream, bool F_bound) {
    TTS_CHECK(g && spec && F && wav && B >= 1 && Fmax >= 2 && iters >= 0, TTS_ERR_INVALID, "bad gl_run arguments");
    TTS_CHECK(!F_bound || F_dev, TTS_ERR_INVALID, "F_bound needs device frame counts");
    TTS_CHECK(mode == TTS_GL_FROM_MEL || mode == TTS_GL_FROM_LINEAR, TTS_ERR_INVALID, "bad mode");
    TTS_CHECK(mode == TTS_GL_FROM_LINEAR || g->pinv, TTS_ERR_INVALID, "mel mode needs inv_mel_basis at create");
    for (int b = 0; b < B; ++b) TTS_CHECK(F[b] >= 2 && F[b] <= Fmax, TTS_ERR_INVALID, "F[b] out of range [2, Fmax]");
    RunCtx c{};
    c.mode = mode; c.spec = spec; c.F = F; c.F_dev = F_dev; c.F_bound = F_bound;
    c.B = B; c.Fmax = Fmax; c.iters = iters;
    c.phase_u = phase_u; c.seed = seed; c.wav = wav;
    c.cs = stream;
    c.s = g->pipeline ? stream : g->stream;
    c.Nmax = (int64_t)g->g.hop * (Fmax - 1);
    c.fstride = (size_t)B * Fmax * g->g.winp;
    c.timed = !g->pipeline;
    TTS_TRY(gl_collect(g));  // the previous pipeline run, if any (its status, timing)
    TTS_TRY(reserve_workspace(g, c));
    // path choice (host values only): small batches fuse the overlap-add into the iteration launch;
    // at most 512 frames in all run the whole loop as one persistent launch
    c.fused = gl_fused_path(g, B, Fmax);
    for (int b = 0; b < B; ++b) c.frames_total += F[b];
    c.persistent = gl_persistent_path(g, B, Fmax, c.frames_total, iters);
    // the launches read the frame counts from F_dev when the persistent loop takes them all; the
    // graph-replayed loops read the handle's own array, which their graphs bake in
    c.Fd = c.persistent && F_dev ? F_dev : g->F.p;
    if (c.Fd == g->F.p) TTS_TRY(stage_counts(g, c));
    TTS_TRY(draw_phases(g, c));
    TTS_TRY(launch_magnitude(g, c));
    TTS_TRY(launch_init(g, c));
    if (c.persistent) TTS_TRY(run_persistent(g, c));
    if (!c.persistent_ran && c.Fd != g->F.p) {  // not placed: the fallbacks' graphs read the handle's array
        TTS_TRY(stage_counts(g, c));
        c.Fd = c.ia.F = c.fa.F = g->F.p;
    }
    if (!c.persistent_ran && iters > 0) TTS_TRY(run_graph_loop(g, c));
    TTS_TRY(finish(g, c));
    return record_last(g, c);
}

}  // namespace tts

extern "C" {

tts_status tts_gl_run(tts_gl* g, int mode, const float* spec, const int32_t* F, int B, int Fmax,
                      const double* phase_u, uint64_t seed, int iters, double* wav, void* stream) {
    return tts::gl_run_dev(g, mode, spec, F, nullptr, B, Fmax, phase_u, seed, iters, wav, static_cast<hipStream_t>(stream));
}

tts_status tts_gl_profile(tts_gl* g, int reps, float* kernel_ms, int n_kernels) {
    TTS_CHECK(g && kernel_ms && n_kernels >= TTS_GL_KERNELS && reps >= 1, TTS_ERR_INVALID, "bad profile arguments");
    TTS_CHECK(g->have_last, TTS_ERR_INVALID, "tts_gl_profile needs a previous tts_gl_run");
    TTS_TRY(gl_collect(g));
    hipStream_t s = g->stream;
    hipEvent_t ev[3];
    for (auto& e : ev) TTS_HIP(hipEventCreate(&e));
    double it_ms = 0.0, ola_ms = 0.0;
    for (int r = 0; r < reps; ++r) {
        // one GL iteration as tts_gl_run launches it: overlap-add -> per-frame STFT/iSTFT
        FinArgs f = g->last_fin;
        f.frames = g->frames.p + (r & 1) * g->last_fstride;
        IterArgs a = g->last_iter;
        a.phase_u = nullptr;
        a.next = g->frames.p + ((r + 1) & 1) * g->last_fstride;
        a.prev = f.frames;
        TTS_HIP(hipEventRecord(ev[0], s));
        if (!g->last_fused) launch_ola_frames(f, s);
        TTS_HIP(hipGetLastError());
        TTS_HIP(hipEventRecord(ev[1], s));
        launch_iteration(g->last_fused, g->wave, a, s);
        TTS_HIP(hipGetLastError());
        TTS_HIP(hipEventRecord(ev[2], s));
        TTS_HIP(hipEventSynchronize(ev[2]));
        float a_ms = 0.f, b_ms = 0.f;
        TTS_HIP(hipEventElapsedTime(&b_ms, ev[0], ev[1]));
        TTS_HIP(hipEventElapsedTime(&a_ms, ev[1], ev[2]));
        it_ms += a_ms;
        ola_ms += b_ms;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    kernel_ms[0] = (float)(it_ms / reps);
    kernel_ms[1] = (float)(ola_ms / reps);
    return TTS_OK;
}

}  // extern "C"
