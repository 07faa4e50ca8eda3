// Trainable conv-BN block: the reference's ConvBNBlock (layers/tacotron2.py:9-27), Conv1d(k = 5, padding = 2)
// -> BatchNorm1d -> ReLU | Tanh | nothing -> Dropout, forward with batch statistics and its whole backward.
// The reference uses it as Encoder.convolutions (:52-55, 3 x 512 -> 512, relu) and Postnet.convolutions
// (:30-45, 80 -> 512 -> 512 -> 512 -> 512 -> 80, tanh x 4 then none).
//
// All arithmetic is fp32 except the per-channel sums, which are fp64; every matrix product goes through
// v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain); every reduction has a fixed order and there are no
// floating-point atomics, so two runs on the same operands give the same bits.  Plain launches on the
// caller's stream: no persistent kernel, no polling, no device-wide wait.
//
// Layouts.  x, out, grad_out, grad_x are [B][C][T] as the reference holds them; rows of T floats are read
// and written with 4-byte accesses only (T is arbitrary).  The products read position-major copies with the
// convolution's zero padding written out: xt [B][T + 4][Cin] (row 2 + t = position t, rows 0, 1, T + 2,
// T + 3 zero) and dyt [B][T + 4][Cout].  With them the five taps of position (b, t) are ONE contiguous
// window of 5 * Cin floats starting at row b * (T + 4) + t, so the convolution is a GEMM with K = 5 * Cin
// over overlapping rows, and no load is predicated on t.  Weights: wf [Cout][5][Cin] (forward),
// wb [Cin][5][Cout] with the taps flipped (grad_x).
//
// k order of a product.  K runs tap-major (tap 0..4, channel 0..C-1 inside a tap) in chunks of 16; within a
// chunk, MFMA j (0..3) takes k = j, 4 + j, 8 + j, 12 + j.  A tap's C products are one chain from zero; the five
// chains are added in tap order (a chain of 5 C would lose a bit more).  grad_W reduces over the positions p = b * T + t in
// chunks of CB_KC positions, ascending inside a chunk (4 positions per MFMA), one partial per chunk and tap,
// folded in chunk order.
// Per-channel sums (sum y, sum y^2; sum dz, sum dz * xhat; sum dy) are fp64: a tile is 64 positions of one
// sentence, summed across the wave by a fixed xor tree; the tiles are folded in tile order (b-major) as 16 runs
// of consecutive tiles, the runs added in run order.  The
// variance is sum y^2 / n - mean^2 in fp64, never in fp32.
//
// Launches of a training forward (5): rows (x -> xt), conv (y = xt * wf + bias, [B][Cout][T]), statistics
// partials, statistics fold (mean, invstd, the running buffers in place), normalise + activation + dropout.
// With training == 0 (4): rows, conv, statistics from the running buffers, normalise + activation.
// Launches of a backward (at most 10): dz partials, dz fold (grad_gamma, grad_beta, the two means of dy's
// formula); dy (written as dyt, with its per-tile sums); fold (grad_bias); rows (x -> xt), grad_W partials,
// fold; conv (grad_x = dyt * wb).  A product nobody asked for is not launched.
// The reserve holds y [B][Cout][T], mean [Cout], invstd [Cout] and the dropout scale: xhat, z and the
// activation's derivative are recomputed from y by the arithmetic the forward used.
#include <algorithm>

#include "host_util.h"

namespace tts {
namespace {

typedef float float4a __attribute__((ext_vector_type(4)));

constexpr int CB_TAPS = 5;
constexpr int CB_PAD = 2;
constexpr int CB_KC = 1024;  // positions per reduction chunk of grad_W
constexpr int CB_TU = 8;     // groups of 4 positions per load group of cb_tn_partial_kernel
constexpr int CB_TC = 16;    // channels of an elementwise tile
constexpr int CB_TT = 64;    // positions of an elementwise tile

__device__ __forceinline__ float4a ldg4(const float* p) { return *reinterpret_cast<const float4a*>(p); }
__device__ __forceinline__ void stg4(float* p, float4a v) { *reinterpret_cast<float4a*>(p) = v; }

// the sum over the 64 lanes of a wave, by a fixed xor tree (every lane gets it)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Where a workgroup of an elementwise kernel stands: grid.x = B * ceil(T / 64), grid.y = C / 16; wave w takes
// channels c0 + 4w .. + 3, lane l position t0 + l of sentence b.
struct Tile {
    int b, t0, c0, tile;
};
__device__ __forceinline__ Tile cb_tile(int T) {
    const int ntb = (T + CB_TT - 1) / CB_TT;
    const int b = blockIdx.x / ntb;
    return Tile{b, (int)(blockIdx.x - b * ntb) * CB_TT, (int)blockIdx.y * CB_TC, (int)blockIdx.x};
}

// ------------------------------------------------------------------ weights
struct PackArgs {
    const float *W, *bias, *gamma, *beta;  // W [Cout][Cin][5]
    float *wf, *wb, *pb, *pg, *pbeta;
    int Cin, Cout;
};
__global__ void cb_pack_kernel(const PackArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)a.Cout * a.Cin * CB_TAPS) {
        const int co = (int)(i / (a.Cin * CB_TAPS)), rem = (int)(i - (int64_t)co * a.Cin * CB_TAPS);
        const int ci = rem / CB_TAPS, k = rem - ci * CB_TAPS;
        const float v = a.W[i];
        a.wf[((int64_t)co * CB_TAPS + k) * a.Cin + ci] = v;
        a.wb[((int64_t)ci * CB_TAPS + (CB_TAPS - 1 - k)) * a.Cout + co] = v;
    }
    if (i < a.Cout) {
        a.pb[i] = a.bias[i];
        a.pg[i] = a.gamma[i];
        a.pbeta[i] = a.beta[i];
    }
}

// ------------------------------------------------------------------ [B][C][T] -> [B][T + 4][C], padding rows zero
__global__ __launch_bounds__(256) void cb_rows_kernel(const float* x, float* xt, int C, int T) {
    __shared__ float tile[CB_TT][CB_TC + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile w = cb_tile(T);
    const int t = w.t0 + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = wave * 4 + i;
        tile[lane][c] = t < T ? x[((int64_t)w.b * C + w.c0 + c) * T + t] : 0.f;
    }
    __syncthreads();
    const int tr = threadIdx.x >> 2, c4 = (threadIdx.x & 3) * 4;
    float* base = xt + (int64_t)w.b * (T + 2 * CB_PAD) * C + w.c0 + c4;
    if (w.t0 + tr < T)
        stg4(base + (int64_t)(CB_PAD + w.t0 + tr) * C, float4a{tile[tr][c4], tile[tr][c4 + 1], tile[tr][c4 + 2],
                                                                tile[tr][c4 + 3]});
    if (w.t0 == 0 && tr < 2 * CB_PAD) stg4(base + (int64_t)(tr < CB_PAD ? tr : T + tr) * C, float4a{0.f, 0.f, 0.f, 0.f});
}

// ------------------------------------------------------------------ out[b][m][t] = sum_k W[m][k] win(b, t)[k] + bias[m]
// win(b, t) = the 5 * Cin floats from row b * (T + 4) + t of A.  MFMA A = 16 output channels, B = 16
// positions: lane l ends with channels (l >> 4) * 4 + 0..3 of position l & 15, so 16 lanes store 16
// consecutive t.  A workgroup of four waves takes 64 channels x 128 positions, a wave 32 x 64 (2 x 4 MFMA
// tiles): per 16 k, 6 operand loads of 16 bytes per lane feed 32 MFMAs; the next chunk's operands are loaded
// before the current chunk's MFMAs.
struct ConvArgs {
    const float* A;     // [B][T + 4][Cin]
    const float* W;     // [M][5 * Cin]
    const float* bias;  // [M] or null
    float* out;         // [B][M][T]
    int B, T, Cin, M;
};
__global__ __launch_bounds__(256) void cb_conv_kernel(const ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.B * a.T, K = CB_TAPS * a.Cin;
    const int m0 = blockIdx.y * 64 + (wave & 1) * 32, p0 = blockIdx.x * 128 + (wave >> 1) * 64;
    if (m0 >= a.M || p0 >= N) return;  // (wave-uniform; no barrier below)
    const int kq = (lane >> 4) * 4;
    const float* wp[2];
    const float* xp[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + mt * 16 + (lane & 15);
        wp[mt] = m < a.M ? a.W + (int64_t)m * K + kq : nullptr;
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int p = p0 + pt * 16 + (lane & 15);
        xp[pt] = p < N ? a.A + ((int64_t)p + 2 * CB_PAD * (p / a.T)) * a.Cin + kq : nullptr;
    }
    floatx4 acc[2][4], part[2][4];  // the sum of the finished taps, the running tap
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[mt][pt] = part[mt][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    float4a wv[2], xv[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) wv[mt] = wp[mt] ? ldg4(wp[mt]) : zero;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) xv[pt] = xp[pt] ? ldg4(xp[pt]) : zero;
    for (int k = 0; k < K; k += 16) {
        float4a wn[2], xn[4];
        const bool more = k + 16 < K;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) wn[mt] = (more && wp[mt]) ? ldg4(wp[mt] + k + 16) : zero;
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) xn[pt] = (more && xp[pt]) ? ldg4(xp[pt] + k + 16) : zero;
        __builtin_amdgcn_sched_barrier(0);  // the next chunk's loads are issued before this chunk's MFMAs
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) part[mt][pt] = mfma16x16x4(wv[mt][j], xv[pt][j], part[mt][pt]);
        if ((k + 16) % a.Cin == 0) {  // (uniform) a tap is complete: a chain is Cin long, the taps are added in order
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) {
                    acc[mt][pt] += part[mt][pt];
                    part[mt][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
                }
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) wv[mt] = wn[mt];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) xv[pt] = xn[pt];
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int p = p0 + pt * 16 + (lane & 15);
        if (p >= N) continue;
        const int b = p / a.T, t = p - b * a.T;
        float* o = a.out + (int64_t)b * a.M * a.T + t;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + mt * 16 + (lane >> 4) * 4 + r;
                if (m < a.M) o[(int64_t)m * a.T] = acc[mt][pt][r] + (a.bias ? a.bias[m] : 0.f);
            }
    }
}

// ------------------------------------------------------------------ batch statistics
// P[tile][c][2] = sum y, sum y^2 over the tile's positions of channel c, in fp64.
__global__ __launch_bounds__(256) void cb_stats_partial_kernel(const float* y, int C, int T, double* P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile w = cb_tile(T);
    const int t = w.t0 + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = w.c0 + wave * 4 + i;
        const double v = t < T ? (double)y[((int64_t)w.b * C + c) * T + t] : 0.0;
        const double s1 = wave_sum(v), s2 = wave_sum(v * v);
        if (lane == 0) {
            double* p = P + ((int64_t)w.tile * C + c) * 2;
            p[0] = s1;
            p[1] = s2;
        }
    }
}

// The fold of per-tile partials P[tile][c][NV] of the 16 channels of a workgroup (256 threads): thread
// (run j = tid >> 4, channel tid & 15) adds the tiles of run j (consecutive tiles, in order), the 16 runs are
// added in run order by the threads of run 0, which get the sums; the others get nothing to do (false).
constexpr int CB_RUNS = 16;
template <int NV>
__device__ __forceinline__ bool cb_fold_tiles(const double* P, int C, int ntiles, double (&sum)[NV]) {
    __shared__ double red[NV][CB_RUNS][CB_TC];
    const int cl = threadIdx.x & 15, j = threadIdx.x >> 4, c = blockIdx.x * CB_TC + cl;
    const int len = (ntiles + CB_RUNS - 1) / CB_RUNS, i1 = min(ntiles, (j + 1) * len);
    double s[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] = 0.0;
    for (int i = j * len; i < i1; ++i)
#pragma unroll
        for (int v = 0; v < NV; ++v) s[v] += P[((int64_t)i * C + c) * NV + v];
#pragma unroll
    for (int v = 0; v < NV; ++v) red[v][j][cl] = s[v];
    __syncthreads();
    if (j != 0) return false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        sum[v] = red[v][0][cl];
        for (int r = 1; r < CB_RUNS; ++r) sum[v] += red[v][r][cl];
    }
    return true;
}

// stat = mean [C] | invstd [C] | dropout scale.  training: from the partials folded in tile order, and the
// running buffers move; else from the running buffers.
struct StatArgs {
    const double* P;
    float *stat, *rmean, *rvar;
    int C, ntiles, training;
    double n, momentum, eps;
    float scale;
};
__global__ __launch_bounds__(256) void cb_stats_fold_kernel(const StatArgs a) {
    const int c = blockIdx.x * CB_TC + (threadIdx.x & 15);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.stat[2 * a.C] = a.scale;
    double s[2];
    if (!cb_fold_tiles<2>(a.P, a.C, a.training ? a.ntiles : 0, s)) return;
    double mean, var;
    if (a.training) {
        mean = s[0] / a.n;
        var = fmax(s[1] / a.n - mean * mean, 0.0);
        a.rmean[c] = (float)((1.0 - a.momentum) * (double)a.rmean[c] + a.momentum * mean);
        a.rvar[c] = (float)((1.0 - a.momentum) * (double)a.rvar[c] + a.momentum * var * (a.n / (a.n - 1.0)));
    } else {
        mean = (double)a.rmean[c];
        var = (double)a.rvar[c];
    }
    a.stat[c] = (float)mean;
    a.stat[a.C + c] = (float)(1.0 / sqrt(var + a.eps));
}

__device__ __forceinline__ float cb_act(float z, int act) { return act == 1 ? (z > 0.f ? z : 0.f) : act == 2 ? tanhf(z) : z; }

// out = act(gamma * (y - mean) * invstd + beta) * scale where mask != 0, else +0.0; mask null: everything kept
struct NormArgs {
    const float *y, *stat, *gamma, *beta;
    const uint8_t* mask;
    float* out;
    int C, T, act;
    float scale;
};
__global__ __launch_bounds__(256) void cb_norm_act_kernel(const NormArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile w = cb_tile(a.T);
    const int t = w.t0 + lane;
    if (t >= a.T) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = w.c0 + wave * 4 + i;
        const int64_t e = ((int64_t)w.b * a.C + c) * a.T + t;
        const float xhat = (a.y[e] - a.stat[c]) * a.stat[a.C + c];
        const float v = cb_act(a.gamma[c] * xhat + a.beta[c], a.act) * a.scale;
        a.out[e] = (!a.mask || a.mask[e]) ? v : 0.f;
    }
}

// ------------------------------------------------------------------ backward, elementwise part
struct DzArgs {
    const float *y, *stat, *gamma, *beta, *gout, *coef;
    const uint8_t* mask;
    double* P;
    float* dyt;
    int C, T, act;
};
// dz = grad_out * mask * scale * act'(z), and xhat
__device__ __forceinline__ float cb_dz(const DzArgs& a, int c, int64_t e, float* xhat) {
    const float xh = (a.y[e] - a.stat[c]) * a.stat[a.C + c];
    const float z = a.gamma[c] * xh + a.beta[c];
    float d = a.mask[e] ? a.gout[e] * a.stat[2 * a.C] : 0.f;
    if (a.act == 1) d = z > 0.f ? d : 0.f;
    if (a.act == 2) {
        const float th = tanhf(z);
        d = d * (1.f - th * th);
    }
    *xhat = xh;
    return d;
}

// P[tile][c][2] = sum dz, sum dz * xhat
__global__ __launch_bounds__(256) void cb_dz_partial_kernel(const DzArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile w = cb_tile(a.T);
    const int t = w.t0 + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = w.c0 + wave * 4 + i;
        float xh = 0.f, d = 0.f;
        if (t < a.T) d = cb_dz(a, c, ((int64_t)w.b * a.C + c) * a.T + t, &xh);
        const double s1 = wave_sum((double)d), s2 = wave_sum((double)d * (double)xh);
        if (lane == 0) {
            double* p = a.P + ((int64_t)w.tile * a.C + c) * 2;
            p[0] = s1;
            p[1] = s2;
        }
    }
}

// grad_beta = sum dz, grad_gamma = sum dz * xhat (either may be null); coef = sum dz / n [C] | sum dz xhat / n [C]
__global__ __launch_bounds__(256) void cb_dz_fold_kernel(const double* P, int C, int ntiles, double n, float* coef,
                                                         float* grad_gamma, float* grad_beta) {
    const int c = blockIdx.x * CB_TC + (threadIdx.x & 15);
    double s[2];
    if (!cb_fold_tiles<2>(P, C, ntiles, s)) return;
    const double s1 = s[0], s2 = s[1];
    if (grad_beta) grad_beta[c] = (float)s1;
    if (grad_gamma) grad_gamma[c] = (float)s2;
    coef[c] = (float)(s1 / n);
    coef[C + c] = (float)(s2 / n);
}

// dy = gamma * invstd * (dz - coef0 - xhat * coef1), written position-major with the padding rows (dyt);
// P[tile][c] = sum dy over the tile
__global__ __launch_bounds__(256) void cb_dy_kernel(const DzArgs a) {
    __shared__ float tile[CB_TT][CB_TC + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Tile w = cb_tile(a.T);
    const int t = w.t0 + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cl = wave * 4 + i, c = w.c0 + cl;
        float dy = 0.f;
        if (t < a.T) {
            float xh;
            const float d = cb_dz(a, c, ((int64_t)w.b * a.C + c) * a.T + t, &xh);
            dy = (a.gamma[c] * a.stat[a.C + c]) * ((d - a.coef[c]) - xh * a.coef[a.C + c]);
        }
        tile[lane][cl] = dy;
        const double s = wave_sum((double)dy);
        if (lane == 0) a.P[(int64_t)w.tile * a.C + c] = s;
    }
    __syncthreads();
    const int tr = threadIdx.x >> 2, c4 = (threadIdx.x & 3) * 4;
    float* base = a.dyt + (int64_t)w.b * (a.T + 2 * CB_PAD) * a.C + w.c0 + c4;
    if (w.t0 + tr < a.T)
        stg4(base + (int64_t)(CB_PAD + w.t0 + tr) * a.C, float4a{tile[tr][c4], tile[tr][c4 + 1], tile[tr][c4 + 2],
                                                                  tile[tr][c4 + 3]});
    if (w.t0 == 0 && tr < 2 * CB_PAD)
        stg4(base + (int64_t)(tr < CB_PAD ? tr : a.T + tr) * a.C, float4a{0.f, 0.f, 0.f, 0.f});
}

// dst[c] = the fold of P[tile][c]
__global__ __launch_bounds__(256) void cb_fold1_kernel(const double* P, int C, int ntiles, float* dst) {
    double s[1];
    if (cb_fold_tiles<1>(P, C, ntiles, s)) dst[blockIdx.x * CB_TC + (threadIdx.x & 15)] = (float)s[0];
}

// ------------------------------------------------------------------ grad_W partials
// P[split][tap][co][ci] = sum over the chunk's positions p = (b, t) of dy[b][co][t] * x[b][ci][t + tap - 2]
//                       = sum of dyt[row + 2][co] * xt[row + tap][ci], row = p + 4 b.
// One wave per 64 x 64 tile, chunk and tap.  Per 4 positions a lane loads 16 bytes of each operand: component
// jm of the dyt load is channel m0 + 4 (l & 15) + jm, i.e. the 64 channels form 4 interleaved MFMA tiles, the
// same on the xt side, so a lane's four results along ci are adjacent and stored as 16 bytes.
struct TnArgs {
    const float *dyt, *xt;
    float* P;
    int B, T, Cout, Cin;
};
__global__ __launch_bounds__(64) void cb_tn_partial_kernel(const TnArgs a) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int split = blockIdx.z / CB_TAPS, tap = blockIdx.z - split * CB_TAPS;
    const int am = m0 + 4 * (lane & 15), bn = n0 + 4 * (lane & 15), kl = lane >> 4;
    const bool mok = am < a.Cout, nok = bn < a.Cin;  // (Cout, Cin multiples of 16: a group of 4 is in or out)
    floatx4 acc[4][4];
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    const int N = a.B * a.T;
    const int k1 = min(N, (split + 1) * CB_KC);
    for (int k0 = split * CB_KC; k0 < k1; k0 += 4 * CB_TU) {
        float4a av[CB_TU], bv[CB_TU];
#pragma unroll
        for (int u = 0; u < CB_TU; ++u) {
            const int p = k0 + 4 * u + kl;
            av[u] = bv[u] = zero;
            if (p >= k1) continue;
            const int64_t row = (int64_t)p + 2 * CB_PAD * (p / a.T);
            if (mok) av[u] = ldg4(a.dyt + (row + CB_PAD) * a.Cout + am);
            if (nok) bv[u] = ldg4(a.xt + (row + tap) * a.Cin + bn);
        }
        __builtin_amdgcn_sched_barrier(0);  // the loads stay together, ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < CB_TU; ++u)
#pragma unroll
            for (int jm = 0; jm < 4; ++jm)
#pragma unroll
                for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = mfma16x16x4(av[u][jm], bv[u][jn], acc[jm][jn]);
    }
    if (!nok) return;
    float* p = a.P + ((int64_t)split * CB_TAPS + tap) * a.Cout * a.Cin;
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * ((lane >> 4) * 4 + r) + jm;
            if (m < a.Cout)
                stg4(p + (int64_t)m * a.Cin + bn, float4a{acc[jm][0][r], acc[jm][1][r], acc[jm][2][r], acc[jm][3][r]});
        }
}

// grad_W[co][ci][tap] = P[0][tap][co][ci] + P[1][tap][co][ci] + ... in chunk order
__global__ void cb_fold_w_kernel(const float* P, int nsplit, int64_t cc, float* grad_W) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cc) return;
#pragma unroll
    for (int tap = 0; tap < CB_TAPS; ++tap) {
        float s = P[tap * cc + e];
        for (int k = 1; k < nsplit; ++k) s += P[((int64_t)k * CB_TAPS + tap) * cc + e];
        grad_W[e * CB_TAPS + tap] = s;
    }
}

}  // namespace
}  // namespace tts

struct tts_convbn {
    int Cin = 0, Cout = 0, act = 0;
    bool have_weights = false;
    tts::DeviceBuf<float> wf, wb, bias, gamma, beta;
    tts::DeviceBuf<float> xt, dyt, y, stat, coef, wpart;
    tts::DeviceBuf<double> cpart;
};

namespace tts {
namespace {

int cb_ntiles(int B, int T) { return B * ((T + CB_TT - 1) / CB_TT); }

tts_status check_shape(const tts_convbn* h, int B, int T, const char* what) {
    TTS_CHECK(h, TTS_ERR_INVALID, std::string(what) + ": null handle");
    TTS_CHECK(h->have_weights, TTS_ERR_INVALID, std::string(what) + ": tts_convbn_set_weights has not been called");
    TTS_CHECK(B > 0 && T > 0, TTS_ERR_INVALID, std::string(what) + ": B and T must be positive");
    TTS_CHECK((int64_t)B * (T + 2 * CB_PAD) < (1 << 23), TTS_ERR_INVALID, std::string(what) + ": B * T too large");
    return TTS_OK;
}

dim3 tile_grid(int B, int T, int C) { return dim3((unsigned)cb_ntiles(B, T), (unsigned)(C / CB_TC)); }

tts_status rows(const float* x, float* xt, int B, int T, int C, hipStream_t s) {
    hipLaunchKernelGGL(cb_rows_kernel, tile_grid(B, T, C), dim3(256), 0, s, x, xt, C, T);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status conv(const float* A, const float* W, const float* bias, float* out, int B, int T, int Cin, int M,
                hipStream_t s) {
    const ConvArgs c{A, W, bias, out, B, T, Cin, M};
    hipLaunchKernelGGL(cb_conv_kernel, dim3((unsigned)((B * T + 127) / 128), (unsigned)((M + 63) / 64)), dim3(256), 0, s,
                       c);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_convbn_create(int cin, int cout, int kernel_size, int act, tts_convbn** out) {
    TTS_CHECK(out, TTS_ERR_INVALID, "convbn_create: null argument");
    TTS_CHECK(act >= 0 && act <= 2, TTS_ERR_INVALID, "convbn_create: act must be 0 (none), 1 (relu) or 2 (tanh)");
    TTS_CHECK(kernel_size == CB_TAPS, TTS_ERR_UNSUPPORTED, "convbn_create: kernel_size must be 5");
    TTS_CHECK(cin > 0 && cout > 0 && cin % 16 == 0 && cout % 16 == 0 && cin <= 8192 && cout <= 8192,
              TTS_ERR_UNSUPPORTED, "convbn_create: cin and cout must be positive multiples of 16 (at most 8192)");
    tts_convbn* h = new tts_convbn();
    h->Cin = cin;
    h->Cout = cout;
    h->act = act;
    *out = h;
    return TTS_OK;
}

void tts_convbn_destroy(tts_convbn* h) {
    if (!h) return;
    for (float* p : {h->wf.p, h->wb.p, h->bias.p, h->gamma.p, h->beta.p, h->xt.p, h->dyt.p, h->y.p, h->stat.p,
                     h->coef.p, h->wpart.p})
        if (p) (void)hipFree(p);
    if (h->cpart.p) (void)hipFree(h->cpart.p);
    delete h;
}

tts_status tts_convbn_set_weights(tts_convbn* h, const float* W, const float* bias, const float* gamma,
                                  const float* beta, void* stream) {
    TTS_CHECK(h && W && bias && gamma && beta, TTS_ERR_INVALID, "convbn_set_weights: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)h->Cout * h->Cin * CB_TAPS;
    TTS_TRY(h->wf.reserve((size_t)n));
    TTS_TRY(h->wb.reserve((size_t)n));
    TTS_TRY(h->bias.reserve((size_t)h->Cout));
    TTS_TRY(h->gamma.reserve((size_t)h->Cout));
    TTS_TRY(h->beta.reserve((size_t)h->Cout));
    const PackArgs p{W, bias, gamma, beta, h->wf.p, h->wb.p, h->bias.p, h->gamma.p, h->beta.p, h->Cin, h->Cout};
    hipLaunchKernelGGL(cb_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    TTS_HIP(hipGetLastError());
    h->have_weights = true;
    return TTS_OK;
}

int64_t tts_convbn_reserve_floats(const tts_convbn* h, int B, int T) {
    if (!h || B <= 0 || T <= 0) return 0;
    return (int64_t)B * h->Cout * T + 2 * (int64_t)h->Cout + 1;
}

tts_status tts_convbn_forward(tts_convbn* h, const float* x, int B, int T, const uint8_t* mask, float p_keep_scale,
                              float* running_mean, float* running_var, double momentum, double eps, int training,
                              float* out, float* reserve, void* stream) {
    TTS_TRY(check_shape(h, B, T, "convbn_forward"));
    TTS_CHECK(x && out, TTS_ERR_INVALID, "convbn_forward: null x or out");
    TTS_CHECK(running_mean && running_var, TTS_ERR_INVALID, "convbn_forward: null running statistics");
    TTS_CHECK(!training || mask, TTS_ERR_INVALID, "convbn_forward: null mask in training");
    TTS_CHECK(!training || (int64_t)B * T > 1, TTS_ERR_INVALID,
              "convbn_forward: batch statistics need more than one value per channel");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Cin = h->Cin, Cout = h->Cout, ntiles = cb_ntiles(B, T);
    const int64_t ny = (int64_t)B * Cout * T;
    TTS_TRY(h->xt.reserve((size_t)B * (T + 2 * CB_PAD) * Cin));
    float *y = reserve, *stat = reserve ? reserve + ny : nullptr;
    if (!training || !reserve) {
        TTS_TRY(h->y.reserve((size_t)ny));
        TTS_TRY(h->stat.reserve((size_t)(2 * Cout + 1)));
        y = h->y.p;
        stat = h->stat.p;
    }
    if (training) TTS_TRY(h->cpart.reserve((size_t)ntiles * Cout * 2));
    TTS_TRY(rows(x, h->xt.p, B, T, Cin, s));
    TTS_TRY(conv(h->xt.p, h->wf.p, h->bias.p, y, B, T, Cin, Cout, s));
    if (training) {
        hipLaunchKernelGGL(cb_stats_partial_kernel, tile_grid(B, T, Cout), dim3(256), 0, s, y, Cout, T, h->cpart.p);
        TTS_HIP(hipGetLastError());
    }
    const float scale = training ? p_keep_scale : 1.f;
    const StatArgs st{h->cpart.p, stat,     running_mean, running_var, Cout, ntiles, training, (double)B * T,
                      momentum,   eps,      scale};
    hipLaunchKernelGGL(cb_stats_fold_kernel, dim3((unsigned)(Cout / CB_TC)), dim3(256), 0, s, st);
    TTS_HIP(hipGetLastError());
    const NormArgs n{y, stat, h->gamma.p, h->beta.p, training ? mask : nullptr, out, Cout, T, h->act, scale};
    hipLaunchKernelGGL(cb_norm_act_kernel, tile_grid(B, T, Cout), dim3(256), 0, s, n);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status tts_convbn_backward(tts_convbn* h, const float* x, int B, int T, const float* reserve, const uint8_t* mask,
                               const float* grad_out, float* grad_x, float* grad_W, float* grad_bias, float* grad_gamma,
                               float* grad_beta, void* stream) {
    TTS_TRY(check_shape(h, B, T, "convbn_backward"));
    TTS_CHECK(x && reserve && mask && grad_out, TTS_ERR_INVALID, "convbn_backward: null x, reserve, mask or grad_out");
    TTS_CHECK((int64_t)B * T > 1, TTS_ERR_INVALID, "convbn_backward: no training forward has this shape");
    if (!grad_x && !grad_W && !grad_bias && !grad_gamma && !grad_beta) return TTS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Cin = h->Cin, Cout = h->Cout, ntiles = cb_ntiles(B, T);
    const int64_t ny = (int64_t)B * Cout * T;
    const int nsplit = (B * T + CB_KC - 1) / CB_KC;
    const bool need_dy = grad_x || grad_W || grad_bias;
    TTS_TRY(h->cpart.reserve((size_t)ntiles * Cout * 2));
    TTS_TRY(h->coef.reserve((size_t)(2 * Cout)));
    if (need_dy) TTS_TRY(h->dyt.reserve((size_t)B * (T + 2 * CB_PAD) * Cout));
    if (grad_W) {
        TTS_TRY(h->xt.reserve((size_t)B * (T + 2 * CB_PAD) * Cin));
        TTS_TRY(h->wpart.reserve((size_t)nsplit * CB_TAPS * Cout * Cin));
    }
    const DzArgs d{reserve, reserve + ny, h->gamma.p, h->beta.p, grad_out, h->coef.p, mask, h->cpart.p, h->dyt.p, Cout,
                   T,       h->act};
    hipLaunchKernelGGL(cb_dz_partial_kernel, tile_grid(B, T, Cout), dim3(256), 0, s, d);
    TTS_HIP(hipGetLastError());
    hipLaunchKernelGGL(cb_dz_fold_kernel, dim3((unsigned)(Cout / CB_TC)), dim3(256), 0, s, h->cpart.p, Cout, ntiles,
                       (double)B * T, h->coef.p, grad_gamma, grad_beta);
    TTS_HIP(hipGetLastError());
    if (!need_dy) return TTS_OK;
    hipLaunchKernelGGL(cb_dy_kernel, tile_grid(B, T, Cout), dim3(256), 0, s, d);
    TTS_HIP(hipGetLastError());
    if (grad_bias) {
        hipLaunchKernelGGL(cb_fold1_kernel, dim3((unsigned)(Cout / CB_TC)), dim3(256), 0, s, h->cpart.p, Cout,
                           ntiles, grad_bias);
        TTS_HIP(hipGetLastError());
    }
    if (grad_W) {
        TTS_TRY(rows(x, h->xt.p, B, T, Cin, s));
        const TnArgs t{h->dyt.p, h->xt.p, h->wpart.p, B, T, Cout, Cin};
        hipLaunchKernelGGL(cb_tn_partial_kernel,
                           dim3((unsigned)((Cin + 63) / 64), (unsigned)((Cout + 63) / 64), (unsigned)(nsplit * CB_TAPS)),
                           dim3(64), 0, s, t);
        TTS_HIP(hipGetLastError());
        const int64_t cc = (int64_t)Cout * Cin;
        hipLaunchKernelGGL(cb_fold_w_kernel, dim3((unsigned)((cc + 255) / 256)), dim3(256), 0, s, h->wpart.p, nsplit, cc,
                           grad_W);
        TTS_HIP(hipGetLastError());
    }
    if (grad_x) TTS_TRY(conv(h->dyt.p, h->wb.p, nullptr, grad_x, B, T, Cout, Cin, s));
    return TTS_OK;
}

}  // extern "C"
