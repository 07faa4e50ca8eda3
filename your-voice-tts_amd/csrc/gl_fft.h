// Device-only float64 FFT and complex helpers shared by the Griffin-Lim synthesis kernels
// (griffin_lim.hip) and the analysis kernels (audio_analysis.hip).
#pragma once
#include "gl_handle.h"

namespace tts {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
__device__ __forceinline__ double2 cconj(double2 a) { return double2{a.x, -a.y}; }

// Per-thread twiddles of the four twiddled Stockham passes (Ns = 4, 16, 64, 256): loaded once per
// kernel with the other operands, so the FFT passes wait only on LDS.
struct FftTw {
    double2 w[4][3];
};
__device__ __forceinline__ FftTw load_fft_tw(const double2* __restrict__ tw) {
    FftTw t;
    const int j = threadIdx.x;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int Ns = 4 << (2 * p);
        const int k = j & (Ns - 1);
#pragma unroll
        for (int r = 1; r < 4; ++r) t.w[p][r - 1] = tw[k * r * (512 / Ns)];
    }
    return t;
}

// Stockham radix-4, 5 passes, 256 threads x 1 butterfly.  Returns the buffer holding the result.
template <bool INV>
__device__ double2* fft1024(double2* src, double2* dst, const FftTw& tw) {
    const int j = threadIdx.x;
#pragma unroll
    for (int Ns = 1, p = -1; Ns < NH; Ns *= 4, ++p) {
        const int k = j & (Ns - 1);
        double2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = src[j + r * 256];
        if (Ns > 1) {
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                double2 w = tw.w[p][r - 1];
                if (INV) w = cconj(w);
                v[r] = cmul(v[r], w);
            }
        }
        const double2 a0 = double2{v[0].x + v[2].x, v[0].y + v[2].y};
        const double2 a1 = double2{v[0].x - v[2].x, v[0].y - v[2].y};
        const double2 a2 = double2{v[1].x + v[3].x, v[1].y + v[3].y};
        const double2 a3 = double2{v[1].x - v[3].x, v[1].y - v[3].y};
        // -i*a3 = (a3.y, -a3.x); +i*a3 = (-a3.y, a3.x)
        const double2 m3 = INV ? double2{-a3.y, a3.x} : double2{a3.y, -a3.x};
        const int idxD = (j / Ns) * Ns * 4 + k;
        dst[idxD] = double2{a0.x + a2.x, a0.y + a2.y};
        dst[idxD + Ns] = double2{a1.x + m3.x, a1.y + m3.y};
        dst[idxD + 2 * Ns] = double2{a0.x - a2.x, a0.y - a2.y};
        dst[idxD + 3 * Ns] = double2{a1.x - m3.x, a1.y - m3.y};
        __syncthreads();
        double2* t = src;
        src = dst;
        dst = t;
    }
    return src;
}

// np.pad(..., mode='reflect') index map for a signal of length N (any overhang).
__device__ __forceinline__ int reflect_idx(int p, int N) {
    if ((unsigned)p < (unsigned)N) return p;  // interior: no division
    if (N == 1) return 0;
    const int period = 2 * (N - 1);
    int pp = p % period;
    if (pp < 0) pp += period;
    return pp < N ? pp : period - pp;
}

}  // namespace tts
