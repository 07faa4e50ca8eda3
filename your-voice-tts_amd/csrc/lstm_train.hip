// Trainable single-layer LSTM (one or two directions): forward that keeps what the backward needs, the
// backward through time, and the weight / input gradients.  The reference runs it as the encoder's
// nn.LSTM(512, 256, batch_first=True, bidirectional=True) on a packed batch (layers/tacotron2.py:56-76).
//
// All arithmetic is fp32; every matrix product goes through v_mfma_f32_16x16x4_f32 (an exact fp32 fma
// chain in k order); every reduction has a fixed order and there are no floating-point atomics, so two
// runs on the same operands give the same bits.  Every dependency of the recurrence is a kernel boundary
// on the caller's stream: no persistent kernel, no polling, no device-wide wait.
//
// Positions.  Sentence b has L_b valid positions.  The valid positions of the batch are numbered
// r = off[b] + t (off = prefix sums of the lengths); rowmap[r] = b * Tmax + t is the row of the padded
// arrays.  The big GEMMs run over r, so padding rows of x and grad_out are never read.
//
// Launches of a forward:  stage (lengths as kernel arguments: no host copy), maps (+ zero the padding
// rows of out, the initial cell state), xi = x W_ih^T + b_ih + b_hh for both directions (nt_gemm), then
// one step launch per time step for both directions: pre = xi + W_hh h_prev (K = H split over the four
// waves of a workgroup, folded through LDS in wave order), gates and cell update in the epilogue.
// h_prev is read from `out` at the direction's previous position, so nothing is carried but c.
// Launches of a backward: stage, maps, one step launch per time step for both directions:
// dh_rec = dpre_prev W_hh (K = 4H over eight waves) for the workgroup's 16 units, then the elementwise
// backward of those units in the epilogue; dpre goes to dG[B][Tmax][D * 4H] (reference gate order), the
// cell gradient is carried per (direction, sentence, unit) by the one lane that owns it.  dpre_prev is
// read from dG at the position the previous launch wrote, so no launch reads what it writes.  After the
// recurrence: bias gradients (column sums of dG), grad_W_ih and grad_W_hh (tn_partial: A^T B reduced over
// the valid positions in chunks of LT_KC rows, one partial per chunk, folded in chunk order), and
// grad_x = dG W_ih (nt_gemm on the transposed weights).
#include <algorithm>
#include <vector>

#include "host_util.h"

namespace tts {
namespace {

typedef float float4a __attribute__((ext_vector_type(4)));

constexpr int LT_STAGE = 512;   // ints per staging launch (kernel-argument block)
constexpr int LT_KC = 512;      // valid positions per reduction chunk of the weight gradients
constexpr int LT_CUS = 256;      // compute units of an MI355X
constexpr int LT_FWD_WAVES = 4;
constexpr int LT_BWD_WAVES = 8;
constexpr int LT_TU = 8;        // groups of 4 positions per load group of lt_tn_partial_kernel
// 16-k chunks per load group of a step kernel: at H = 256 a wave's whole share (H / 16 / 4, 4H / 16 / 8)
constexpr int LT_FWD_KU = 4;
constexpr int LT_BWD_KU = 8;
// most batch tiles (of 16 sentences) per workgroup of a step launch; the backward holds more per tile in registers
constexpr int LT_FWD_BT = 4;
constexpr int LT_BWD_BT = 2;

__device__ __forceinline__ float4a ldg4(const float* p) { return *reinterpret_cast<const float4a*>(p); }
__device__ __forceinline__ void stg4(float* p, float4a v) { *reinterpret_cast<float4a*>(p) = v; }

// ------------------------------------------------------------------ staging and maps
struct StageArgs {
    int* dst;
    int n;
    int v[LT_STAGE];
};
__global__ void lt_stage_kernel(const StageArgs a) {
    for (int i = threadIdx.x; i < a.n; i += blockDim.x) a.dst[i] = a.v[i];
}

// meta: lens [B] | off [B + 1] | rowmap [B * Tmax] | prev_f [B * Tmax] | prev_r [B * Tmax]
// prev_*[r]: the padded row the direction visited before row r (t - 1 forward, t + 1 reverse), or -1 - b
// at the direction's first position (the initial state of sentence b).
struct MapArgs {
    int* meta;
    int B, Tmax;
};
__global__ void lt_maps_kernel(const MapArgs a) {
    const int* lens = a.meta;
    int* off = a.meta + a.B;
    if (threadIdx.x == 0) {
        int s = 0;
        for (int b = 0; b < a.B; ++b) {
            off[b] = s;
            s += lens[b];
        }
        off[a.B] = s;
    }
    __threadfence_block();
    __syncthreads();
    const int n = a.B * a.Tmax;
    int* rowmap = off + a.B + 1;
    int* prev_f = rowmap + n;
    int* prev_r = prev_f + n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int b = i / a.Tmax, t = i - b * a.Tmax, L = lens[b];
        if (t >= L) continue;
        const int r = off[b] + t;
        rowmap[r] = i;
        prev_f[r] = t == 0 ? -1 - b : i - 1;
        prev_r[r] = t == L - 1 ? -1 - b : i + 1;
    }
}

// +0.0 on the rows t >= L_b of a [B][Tmax][width] array (width a multiple of 4)
__global__ void lt_zero_pad_kernel(float* p, int width, const int* lens, int Tmax) {
    const int row = blockIdx.x, b = row / Tmax, t = row - b * Tmax;
    if (t < lens[b]) return;
    float* q = p + (int64_t)row * width;
    for (int i = threadIdx.x * 4; i < width; i += blockDim.x * 4) stg4(q + i, float4a{0.f, 0.f, 0.f, 0.f});
}

// dst[i] = src ? src[i] : 0
__global__ void lt_copy_or_zero_kernel(float* dst, const float* src, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src ? src[i] : 0.f;
}

// ------------------------------------------------------------------ weights
// From the reference layout (w_ih [4H][I], w_hh [4H][H], biases [4H]; gate rows i, f, g, o) of direction d:
//   whh_g [D][H * 4][H]   row u * 4 + gate = w_hh row gate * H + u: a 16-row tile holds 4 units' gates
//   whh_t [D][H][4H]      w_hh transposed (the backward recurrence)
//   wih   [D * 4H][I]     both directions stacked (xi, one GEMM)
//   wih_t [I][D * 4H]     its transpose (grad_x)
//   bias  [D * 4H]        b_ih + b_hh
struct PackArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float *whh_g, *whh_t, *wih, *wih_t, *bias;
    int I, H, D, d;
};
__global__ void lt_pack_kernel(const PackArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int G = 4 * a.H;
    if (i < (int64_t)G * a.H) {
        const int n = (int)(i / a.H), k = (int)(i - (int64_t)n * a.H);
        const int gate = n / a.H, u = n - gate * a.H;
        const float v = a.w_hh[i];
        a.whh_g[((int64_t)a.d * G + u * 4 + gate) * a.H + k] = v;
        a.whh_t[((int64_t)a.d * a.H + k) * G + n] = v;
    }
    if (i < (int64_t)G * a.I) {
        const int n = (int)(i / a.I), k = (int)(i - (int64_t)n * a.I);
        const float v = a.w_ih[i];
        a.wih[((int64_t)a.d * G + n) * a.I + k] = v;
        a.wih_t[(int64_t)k * a.D * G + a.d * G + n] = v;
    }
    if (i < G) a.bias[a.d * G + i] = a.b_ih[i] + a.b_hh[i];
}

// ------------------------------------------------------------------ C = A W^T (+ bias) over the valid rows
// C[map[r]][n] = sum_k A[map[r]][k] W[n][k] + bias[n], r < M.  K a multiple of 16, N of 16.  A workgroup of
// four waves takes 64 rows x 128 columns, a wave 32 x 64 (2 x 4 MFMA tiles): per 16 k, 6 operand loads of
// 16 bytes per lane feed 32 MFMAs; the next chunk's operands are loaded before the current chunk's MFMAs.
struct NtArgs {
    const float* A;
    int64_t lda;
    const int* map;
    const float* W;
    int64_t ldw;
    const float* bias;
    float* C;
    int64_t ldc;
    int M, N, K;
};
__global__ __launch_bounds__(256) void lt_nt_gemm_kernel(const NtArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 64 + (wave & 1) * 32, n0 = blockIdx.x * 128 + (wave >> 1) * 64;
    if (m0 >= a.M || n0 >= a.N) return;  // (wave-uniform; no barrier below)
    const int kq = (lane >> 4) * 4;
    const float* ap[2];
    const float* wp[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int r = m0 + mt * 16 + (lane & 15);
        ap[mt] = r < a.M ? a.A + (int64_t)a.map[r] * a.lda + kq : nullptr;
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + nt * 16 + (lane & 15);
        wp[nt] = n < a.N ? a.W + (int64_t)n * a.ldw + kq : nullptr;
    }
    floatx4 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    float4a av[2], wv[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) av[mt] = ap[mt] ? ldg4(ap[mt]) : zero;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) wv[nt] = wp[nt] ? ldg4(wp[nt]) : zero;
    for (int k = 0; k < a.K; k += 16) {
        float4a an[2], wn[4];
        const bool more = k + 16 < a.K;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) an[mt] = (more && ap[mt]) ? ldg4(ap[mt] + k + 16) : zero;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wn[nt] = (more && wp[nt]) ? ldg4(wp[nt] + k + 16) : zero;
        __builtin_amdgcn_sched_barrier(0);  // the next chunk's loads are issued before this chunk's MFMAs
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma16x16x4(av[mt][j], wv[nt][j], acc[mt][nt]);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) av[mt] = an[mt];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wv[nt] = wn[nt];
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + mt * 16 + (lane >> 4) * 4 + r;
            if (row >= a.M) continue;
            float* c = a.C + (int64_t)a.map[row] * a.ldc;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = n0 + nt * 16 + (lane & 15);
                if (n < a.N) c[n] = acc[mt][nt][r] + (a.bias ? a.bias[n] : 0.f);
            }
        }
}

// ------------------------------------------------------------------ the recurrence steps
// Both step kernels are written without data-dependent branches around their loads: a lane that has nothing
// to read (an idle sentence, a row past B, the zero initial state) loads from a valid dummy address (its own
// weight row) and the value is replaced by zero, so every load of a phase is in flight at once: the lengths,
// then the operands together with what the epilogue will read, then the stores.  BT, the batch tiles (of 16
// sentences) per workgroup, is a template parameter chosen from B at launch, so no MFMA is predicated.
//
// lt_kdot: this wave's share of sum_k W[row][k] X[b][k].  MFMA A = 16 weight rows, B = 16 sentences: lane l
// ends with rows (l >> 4) * 4 + 0..3 of sentence l & 15.  The wave takes the 16-k chunks wave, wave + NW,
// ..., KU of them per load group; the workgroup folds the waves in index order.
template <int NW, int BT, int KU>
__device__ __forceinline__ void lt_kdot(const float* wrow, const float* const xrow[BT], const bool xact[BT],
                                        int chunks, int wave, int lane, floatx4 acc[BT]) {
    const int kq = (lane >> 4) * 4;
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = wave; c0 < chunks; c0 += NW * KU) {
        float4a w[KU], x[KU][BT];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int c = c0 + u * NW;
            const bool in = c < chunks;  // (wave-uniform)
            const int off = (in ? c : c0) * 16 + kq;
            w[u] = ldg4(wrow + off);
            w[u] = in ? w[u] : zero;
#pragma unroll
            for (int bt = 0; bt < BT; ++bt) {
                x[u][bt] = ldg4(xrow[bt] + off);
                x[u][bt] = xact[bt] ? x[u][bt] : zero;
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // the loads stay together, ahead of the MFMAs: one round trip
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int bt = 0; bt < BT; ++bt) acc[bt] = mfma16x16x4(w[u][j], x[u][bt][j], acc[bt]);
    }
}

struct FwdArgs {
    const float* whh_g;  // [D][4H][H], rows u * 4 + gate
    const float* xi;     // [B][Tmax][D * 4H]
    const float* h0;     // [D][B][H] or null
    const float* c0;     // [D][B][H] (the reserve's copy, or the handle's)
    float* c;            // [D][B][H], in place
    float* out;          // [B][Tmax][D * H]
    float *h_n, *c_n;    // [D][B][H] or null
    float* rg;           // [B][Tmax][D][H][4] activated gates, or null
    float* rc;           // [B][Tmax][D][H] c_t
    const int* lens;
    int B, Tmax, H, D, s;
};

// Step s: the forward direction at position s, the reverse direction at L_b - 1 - s; sentences with
// s >= L_b are idle.  grid.x = D * H / 4 (a workgroup per 4 units), grid.y = groups of 16 * BT sentences.
// Wave w (< BT) finishes batch tile w.
template <int BT>
__global__ __launch_bounds__(LT_FWD_WAVES * 64) void lt_fwd_step_kernel(const FwdArgs a) {
    constexpr int NW = LT_FWD_WAVES;
    static_assert(NW >= BT, "wave bt finishes batch tile bt");
    __shared__ floatx4 red[NW][BT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = a.H / 4, d = blockIdx.x / tiles, tile = blockIdx.x - d * tiles;
    const int g0 = blockIdx.y * 16 * BT;
    const int64_t G = 4 * (int64_t)a.H;
    const float* wrow = a.whh_g + ((int64_t)d * G + tile * 16 + (lane & 15)) * a.H;
    int Ls[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) Ls[bt] = a.lens[min(g0 + bt * 16 + (lane & 15), a.B - 1)];
    const int eb = g0 + min(wave, BT - 1) * 16 + (lane & 15);
    const int eL = a.lens[min(eb, a.B - 1)];

    const float* xrow[BT];
    bool xact[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) {
        const int b = g0 + bt * 16 + (lane & 15), L = Ls[bt];
        const int t = d ? L - 1 - a.s : a.s;
        const bool act = b < a.B && a.s < L;
        xact[bt] = act && (a.s > 0 || a.h0);
        const float* prev = a.s == 0 ? a.h0 + ((int64_t)d * a.B + b) * a.H
                                     : a.out + (((int64_t)b * a.Tmax + (d ? t + 1 : t - 1)) * a.D + d) * a.H;
        xrow[bt] = xact[bt] ? prev : wrow;
    }
    // what the epilogue reads does not depend on the product: loaded with the operands
    const bool eact = wave < BT && eb < a.B && a.s < eL;
    const int et = d ? eL - 1 - a.s : a.s, u = tile * 4 + (lane >> 4);
    const int64_t pos = (int64_t)eb * a.Tmax + et;
    const int64_t st = ((int64_t)d * a.B + eb) * a.H + u;  // state index
    const float* xq = eact ? a.xi + pos * a.D * G + d * G + u : wrow;
    const float* cq = eact ? (a.s == 0 ? a.c0 : a.c) + st : wrow;
    float xi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) xi[g] = xq[eact ? g * a.H : 0];
    const float cp = *cq;

    floatx4 acc[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) acc[bt] = floatx4{0.f, 0.f, 0.f, 0.f};
    lt_kdot<NW, BT, LT_FWD_KU>(wrow, xrow, xact, a.H / 16, wave, lane, acc);
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) red[wave][bt][lane] = acc[bt];
    __syncthreads();
    if (!eact) return;
    floatx4 p = red[0][wave][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) p += red[w][wave][lane];
    const float ig = sigmoid_cell(p[0] + xi[0]);
    const float fg = sigmoid_cell(p[1] + xi[1]);
    const float gg = tanh_cell(p[2] + xi[2]);
    const float og = sigmoid_cell(p[3] + xi[3]);
    const float c = fg * cp + ig * gg;
    const float h = og * tanh_cell(c);
    a.c[st] = c;
    const int64_t e = (pos * a.D + d) * a.H + u;
    a.out[e] = h;
    if (a.rg) {
        stg4(a.rg + e * 4, float4a{ig, fg, gg, og});
        a.rc[e] = c;
    }
    if (a.s == eL - 1) {
        if (a.h_n) a.h_n[st] = h;
        if (a.c_n) a.c_n[st] = c;
    }
}

struct BwdArgs {
    const float* whh_t;  // [D][H][4H]
    const float* rg;     // activated gates
    const float* rc;     // c_t
    const float* c0;     // [D][B][H] (the reserve's copy)
    const float* gout;   // [B][Tmax][D * H]
    float* dG;           // [B][Tmax][D * 4H]
    float* dc;           // [D][B][H] carried cell gradient, in place
    const int* lens;
    int B, Tmax, H, D, q;
};

// Step q of the backward walk: the forward direction at position L_b - 1 - q, the reverse direction at q.
// grid.x = D * H / 16 (a workgroup per 16 units), grid.y = groups of 16 * BT sentences.
template <int BT>
__global__ __launch_bounds__(LT_BWD_WAVES * 64) void lt_bwd_step_kernel(const BwdArgs a) {
    constexpr int NW = LT_BWD_WAVES;
    static_assert(NW >= BT, "wave bt finishes batch tile bt");
    __shared__ floatx4 red[NW][BT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = a.H / 16, d = blockIdx.x / tiles, tile = blockIdx.x - d * tiles;
    const int g0 = blockIdx.y * 16 * BT;
    const int64_t G = 4 * (int64_t)a.H;
    const float* wrow = a.whh_t + ((int64_t)d * a.H + tile * 16 + (lane & 15)) * G;
    const int64_t ldg = a.D * G;
    int Ls[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) Ls[bt] = a.lens[min(g0 + bt * 16 + (lane & 15), a.B - 1)];
    const int eb = g0 + min(wave, BT - 1) * 16 + (lane & 15);
    const int eL = a.lens[min(eb, a.B - 1)];

    const float* xrow[BT];
    bool xact[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) {
        const int b = g0 + bt * 16 + (lane & 15), L = Ls[bt];
        const int t = d ? a.q : L - 1 - a.q;
        xact[bt] = b < a.B && a.q < L && a.q > 0;
        xrow[bt] = xact[bt] ? a.dG + ((int64_t)b * a.Tmax + (d ? t - 1 : t + 1)) * ldg + d * G : wrow;
    }
    const bool eact = wave < BT && eb < a.B && a.q < eL;
    const int et = d ? a.q : eL - 1 - a.q, u0 = tile * 16 + (lane >> 4) * 4;
    const int64_t pos = (int64_t)eb * a.Tmax + et;
    const int64_t e = (pos * a.D + d) * a.H + u0;
    const int64_t st = ((int64_t)d * a.B + eb) * a.H + u0;
    const bool first = d ? et == eL - 1 : et == 0;  // c_{t-1} in the direction's forward order
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    const float4a go = ldg4(eact ? a.gout + e : wrow);
    const float4a c = ldg4(eact ? a.rc + e : wrow);
    const float4a cp = ldg4(!eact ? wrow : first ? a.c0 + st : a.rc + e + (d ? 1 : -1) * (int64_t)a.D * a.H);
    float4a dcb = ldg4(eact && a.q > 0 ? a.dc + st : wrow);
    dcb = a.q > 0 ? dcb : zero;
    float4a gate[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) gate[r] = ldg4(eact ? a.rg + (e + r) * 4 : wrow);  // i, f, g, o

    floatx4 acc[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) acc[bt] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (a.q > 0) lt_kdot<NW, BT, LT_BWD_KU>(wrow, xrow, xact, (int)(G / 16), wave, lane, acc);
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) red[wave][bt][lane] = acc[bt];
    __syncthreads();
    if (!eact) return;
    floatx4 dh = red[0][wave][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) dh += red[w][wave][lane];
    float4a di, df, dg, dO, dcn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4a g = gate[r];
        const float dhr = go[r] + dh[r];
        const float tc = tanh_cell(c[r]);
        const float dc = dcb[r] + dhr * g[3] * (1.f - tc * tc);
        di[r] = dc * g[2] * (g[0] * (1.f - g[0]));
        df[r] = dc * cp[r] * (g[1] * (1.f - g[1]));
        dg[r] = dc * g[0] * (1.f - g[2] * g[2]);
        dO[r] = dhr * tc * (g[3] * (1.f - g[3]));
        dcn[r] = dc * g[1];
    }
    stg4(a.dc + st, dcn);
    float* o = a.dG + pos * ldg + d * G + u0;
    stg4(o, di);
    stg4(o + a.H, df);
    stg4(o + 2 * a.H, dg);
    stg4(o + 3 * a.H, dO);
}

// ------------------------------------------------------------------ A^T B over the valid positions
// P[split][m][n] = sum over the chunk's positions r of A[amap[r]][acol0 + m] * Bm[brow(r)][n], with
// brow(r) = bmap[r] when >= 0, else row -1 - bmap[r] of B0 (the initial state; zeros when B0 is null).
// One wave per 64 x 64 tile and chunk.  Per 4 positions a lane loads 16 bytes of each operand:
// component jm of A is column m0 + 4 (l & 15) + jm, i.e. the 64 columns form 4 interleaved MFMA tiles,
// the same on the B side, so a lane's four results along n are adjacent and stored as 16 bytes.
struct TnArgs {
    const float* A;
    int64_t lda;
    int acol0;
    const int* amap;
    const float* Bm;
    int64_t ldb;
    int bcol0;
    const int* bmap;
    const float* B0;
    int64_t ldb0;
    float* P;
    int M, N, K;
};
__global__ __launch_bounds__(64) void lt_tn_partial_kernel(const TnArgs a) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, split = blockIdx.z;
    const int am = m0 + 4 * (lane & 15), bn = n0 + 4 * (lane & 15), kl = lane >> 4;
    const bool nok = bn < a.N;
    floatx4 acc[4][4];
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    const int k1 = min(a.K, (split + 1) * LT_KC);
    // LT_TU groups of 4 positions at a time: the map entries, then every operand load, then the MFMAs
    for (int k0 = split * LT_KC; k0 < k1; k0 += 4 * LT_TU) {
        int ar[LT_TU], br[LT_TU];
#pragma unroll
        for (int u = 0; u < LT_TU; ++u) {
            const int r = k0 + 4 * u + kl;
            ar[u] = r < k1 ? a.amap[r] : -1;
            br[u] = r < k1 ? a.bmap[r] : 0;
        }
        float4a av[LT_TU], bv[LT_TU];
#pragma unroll
        for (int u = 0; u < LT_TU; ++u) {
            av[u] = bv[u] = zero;
            if (ar[u] < 0) continue;
            av[u] = ldg4(a.A + (int64_t)ar[u] * a.lda + a.acol0 + am);
            if (!nok) continue;
            if (br[u] >= 0)
                bv[u] = ldg4(a.Bm + (int64_t)br[u] * a.ldb + a.bcol0 + bn);
            else if (a.B0)
                bv[u] = ldg4(a.B0 + (int64_t)(-1 - br[u]) * a.ldb0 + bn);
        }
        __builtin_amdgcn_sched_barrier(0);  // the loads stay together, ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < LT_TU; ++u)
#pragma unroll
            for (int jm = 0; jm < 4; ++jm)
#pragma unroll
                for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = mfma16x16x4(av[u][jm], bv[u][jn], acc[jm][jn]);
    }
    if (!nok) return;
    float* p = a.P + (int64_t)split * a.M * a.N;
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * ((lane >> 4) * 4 + r) + jm;  // < M: M is a multiple of 64
            stg4(p + (int64_t)m * a.N + bn, float4a{acc[jm][0][r], acc[jm][1][r], acc[jm][2][r], acc[jm][3][r]});
        }
}

// Column sums of dG over a chunk's positions: P[split][n].  A workgroup takes 64 columns; wave w sums the
// chunk's positions w, w + 4, ... in order (8 loads in flight), the waves are folded in index order.
__global__ __launch_bounds__(256) void lt_colsum_partial_kernel(const float* dG, int64_t ld, const int* map, int K,
                                                                int N, float* P) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane, split = blockIdx.y;
    const int k1 = min(K, (split + 1) * LT_KC);
    float s = 0.f;
    if (n < N) {
        for (int r0 = split * LT_KC + wave; r0 < k1; r0 += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = r0 + 4 * u;
                v[u] = r < k1 ? dG[(int64_t)map[r] * ld + n] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && n < N) P[(int64_t)split * N + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// dst[e] = P[0][e] + P[1][e] + ... in chunk order; elements [0, half) go to out0 (and dup0), the rest to
// out1 (and dup1); a null destination is skipped.  total, half multiples of 4.
struct FoldArgs {
    const float* P;
    int nsplit;
    int64_t total, half;
    float *out0, *out1, *dup0, *dup1;
};
__global__ void lt_fold_kernel(const FoldArgs a) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e >= a.total) return;
    float4a s = ldg4(a.P + e);
    for (int k = 1; k < a.nsplit; ++k) s += ldg4(a.P + k * a.total + e);
    const bool lo = e < a.half;
    float* o = lo ? a.out0 : a.out1;
    float* o2 = lo ? a.dup0 : a.dup1;
    const int64_t i = lo ? e : e - a.half;
    if (o) stg4(o + i, s);
    if (o2) stg4(o2 + i, s);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace tts

struct tts_lstm {
    int I = 0, H = 0, D = 0;
    bool have_weights = false;
    tts::DeviceBuf<float> whh_g, whh_t, wih, wih_t, bias;
    tts::DeviceBuf<int> meta;
    tts::DeviceBuf<float> xi, dG, state, partial;  // state: c | dc | zero-or-c0 copy, each [D][B][H]
};

namespace tts {
namespace {

tts_status check_batch(const tts_lstm* l, const void* x, const int32_t* lens, int B, int Tmax, const char* what) {
    TTS_CHECK(l && x && lens, TTS_ERR_INVALID, std::string(what) + ": null argument");
    TTS_CHECK(l->have_weights, TTS_ERR_INVALID, std::string(what) + ": tts_lstm_set_weights has not been called");
    TTS_CHECK(B > 0 && Tmax > 0, TTS_ERR_INVALID, std::string(what) + ": B and Tmax must be positive");
    TTS_CHECK((int64_t)B * Tmax < (1 << 28), TTS_ERR_INVALID, std::string(what) + ": B * Tmax too large");
    for (int b = 0; b < B; ++b)
        TTS_CHECK(lens[b] >= 1 && lens[b] <= Tmax, TTS_ERR_INVALID,
                  std::string(what) + ": length " + std::to_string(lens[b]) + " of sentence " + std::to_string(b) +
                      " outside [1, Tmax]");
    return TTS_OK;
}

// lengths to the device (kernel arguments) and the maps; *total = the number of valid positions
tts_status stage_maps(tts_lstm* l, const int32_t* lens, int B, int Tmax, int* total, hipStream_t s) {
    TTS_TRY(l->meta.reserve(2 * (size_t)B + 1 + 3 * (size_t)B * Tmax));
    int sum = 0;
    for (int b0 = 0; b0 < B; b0 += LT_STAGE) {
        StageArgs st;
        st.dst = l->meta.p + b0;
        st.n = std::min(LT_STAGE, B - b0);
        for (int i = 0; i < st.n; ++i) sum += (st.v[i] = lens[b0 + i]);
        for (int i = st.n; i < LT_STAGE; ++i) st.v[i] = 0;
        hipLaunchKernelGGL(lt_stage_kernel, dim3(1), dim3(256), 0, s, st);
        TTS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(lt_maps_kernel, dim3(1), dim3(1024), 0, s, MapArgs{l->meta.p, B, Tmax});
    TTS_HIP(hipGetLastError());
    *total = sum;
    return TTS_OK;
}

// Batch tiles per workgroup of a step launch: the most (a power of two up to `most`) that still leaves the
// launch a workgroup per CU; a step is bound by how many loads a CU keeps in flight, not by its MFMAs.
int step_batch_tiles(int unit_tiles, int B, int most) {
    int bt = most;
    while (bt > 1 && (B <= 8 * bt || (int64_t)unit_tiles * ((B + 16 * bt - 1) / (16 * bt)) < LT_CUS)) bt /= 2;
    return bt;
}

tts_status fold(const float* P, int nsplit, int64_t total, int64_t half, float* out0, float* out1, float* dup0,
                float* dup1, hipStream_t s) {
    const FoldArgs f{P, nsplit, total, half, out0, out1, dup0, dup1};
    hipLaunchKernelGGL(lt_fold_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, f);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_lstm_create(int input_size, int hidden_size, int bidirectional, tts_lstm** out) {
    TTS_CHECK(out, TTS_ERR_INVALID, "lstm_create: null argument");
    TTS_CHECK(input_size > 0 && hidden_size > 0 && input_size % 16 == 0 && hidden_size % 16 == 0, TTS_ERR_UNSUPPORTED,
              "lstm_create: input_size and hidden_size must be positive multiples of 16");
    tts_lstm* l = new tts_lstm();
    l->I = input_size;
    l->H = hidden_size;
    l->D = bidirectional ? 2 : 1;
    *out = l;
    return TTS_OK;
}

void tts_lstm_destroy(tts_lstm* l) {
    if (!l) return;
    for (float* p : {l->whh_g.p, l->whh_t.p, l->wih.p, l->wih_t.p, l->bias.p, l->xi.p, l->dG.p, l->state.p,
                     l->partial.p})
        if (p) (void)hipFree(p);
    if (l->meta.p) (void)hipFree(l->meta.p);
    delete l;
}

tts_status tts_lstm_set_weights(tts_lstm* l, const float* const* w_ih, const float* const* w_hh,
                                const float* const* b_ih, const float* const* b_hh, void* stream) {
    TTS_CHECK(l && w_ih && w_hh && b_ih && b_hh, TTS_ERR_INVALID, "lstm_set_weights: null argument");
    for (int d = 0; d < l->D; ++d)
        TTS_CHECK(w_ih[d] && w_hh[d] && b_ih[d] && b_hh[d], TTS_ERR_INVALID, "lstm_set_weights: null tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t G = 4 * (int64_t)l->H;
    TTS_TRY(l->whh_g.reserve((size_t)(l->D * G * l->H)));
    TTS_TRY(l->whh_t.reserve((size_t)(l->D * l->H * G)));
    TTS_TRY(l->wih.reserve((size_t)(l->D * G * l->I)));
    TTS_TRY(l->wih_t.reserve((size_t)(l->I * l->D * G)));
    TTS_TRY(l->bias.reserve((size_t)(l->D * G)));
    const int64_t n = G * std::max(l->I, l->H);
    for (int d = 0; d < l->D; ++d) {
        const PackArgs p{w_ih[d],     w_hh[d],      b_ih[d],   b_hh[d], l->whh_g.p, l->whh_t.p,
                         l->wih.p,    l->wih_t.p,   l->bias.p, l->I,    l->H,       l->D,       d};
        hipLaunchKernelGGL(lt_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
        TTS_HIP(hipGetLastError());
    }
    l->have_weights = true;
    return TTS_OK;
}

int64_t tts_lstm_reserve_floats(const tts_lstm* l, int B, int Tmax) {
    if (!l || B <= 0 || Tmax <= 0) return 0;
    return (int64_t)B * Tmax * l->D * l->H * 5 + (int64_t)l->D * B * l->H;
}

tts_status tts_lstm_forward(tts_lstm* l, const float* x, const int32_t* lens, int B, int Tmax, const float* h0,
                            const float* c0, float* out, float* h_n, float* c_n, float* reserve, void* stream) {
    TTS_TRY(check_batch(l, x, lens, B, Tmax, "lstm_forward"));
    TTS_CHECK(out, TTS_ERR_INVALID, "lstm_forward: null out");
    TTS_CHECK(aligned16(x) && aligned16(out) && aligned16(h0) && aligned16(c0) && aligned16(reserve), TTS_ERR_INVALID,
              "lstm_forward: x, out, h0, c0 and reserve must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = l->D, H = l->H, I = l->I;
    const int64_t G = 4 * (int64_t)H, BT = (int64_t)B * Tmax, nstate = (int64_t)D * B * H;
    int total = 0, Lmax = 0;
    for (int b = 0; b < B; ++b) Lmax = std::max(Lmax, (int)lens[b]);
    const int64_t ldg = D * G;
    TTS_TRY(l->xi.reserve((size_t)(BT * ldg)));
    TTS_TRY(l->state.reserve((size_t)(3 * nstate)));
    TTS_TRY(stage_maps(l, lens, B, Tmax, &total, s));
    const int* dlens = l->meta.p;
    const int* rowmap = l->meta.p + 2 * B + 1;
    hipLaunchKernelGGL(lt_zero_pad_kernel, dim3((unsigned)BT), dim3(64), 0, s, out, D * H, dlens, Tmax);
    TTS_HIP(hipGetLastError());
    float* rg = reserve;
    float* rc = reserve ? reserve + BT * D * H * 4 : nullptr;
    float* c0copy = reserve ? reserve + BT * D * H * 5 : l->state.p + 2 * nstate;
    hipLaunchKernelGGL(lt_copy_or_zero_kernel, dim3((unsigned)((nstate + 255) / 256)), dim3(256), 0, s, c0copy, c0,
                       (int)nstate);
    TTS_HIP(hipGetLastError());
    const NtArgs g{x, I, rowmap, l->wih.p, I, l->bias.p, l->xi.p, ldg, total, (int)(D * G), I};
    hipLaunchKernelGGL(lt_nt_gemm_kernel, dim3((unsigned)((g.N + 127) / 128), (unsigned)((g.M + 63) / 64)), dim3(256), 0,
                       s, g);
    TTS_HIP(hipGetLastError());
    FwdArgs f{l->whh_g.p, l->xi.p, h0, c0copy, l->state.p, out, h_n, c_n, rg, rc, dlens, B, Tmax, H, D, 0};
    const int bt = step_batch_tiles(D * H / 4, B, LT_FWD_BT);
    const dim3 grid((unsigned)(D * H / 4), (unsigned)((B + 16 * bt - 1) / (16 * bt)));
    const auto step_kernel = bt == 1 ? lt_fwd_step_kernel<1> : bt == 2 ? lt_fwd_step_kernel<2> : lt_fwd_step_kernel<LT_FWD_BT>;
    for (int step = 0; step < Lmax; ++step) {
        f.s = step;
        hipLaunchKernelGGL(step_kernel, grid, dim3(LT_FWD_WAVES * 64), 0, s, f);
    }
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status tts_lstm_backward(tts_lstm* l, const float* x, const int32_t* lens, int B, int Tmax, const float* reserve,
                             const float* out, const float* h0, const float* grad_out, float* grad_x,
                             float* const* grad_w_ih, float* const* grad_w_hh, float* const* grad_b_ih,
                             float* const* grad_b_hh, void* stream) {
    TTS_TRY(check_batch(l, x, lens, B, Tmax, "lstm_backward"));
    TTS_CHECK(reserve && out && grad_out, TTS_ERR_INVALID, "lstm_backward: null reserve, out or grad_out");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = l->D, H = l->H, I = l->I;
    float *gwi[2] = {}, *gwh[2] = {}, *gbi[2] = {}, *gbh[2] = {};
    bool ok = aligned16(x) && aligned16(reserve) && aligned16(out) && aligned16(h0) && aligned16(grad_out) &&
              aligned16(grad_x);
    for (int d = 0; d < D; ++d) {
        gwi[d] = grad_w_ih ? grad_w_ih[d] : nullptr;
        gwh[d] = grad_w_hh ? grad_w_hh[d] : nullptr;
        gbi[d] = grad_b_ih ? grad_b_ih[d] : nullptr;
        gbh[d] = grad_b_hh ? grad_b_hh[d] : nullptr;
        ok = ok && aligned16(gwi[d]) && aligned16(gwh[d]) && aligned16(gbi[d]) && aligned16(gbh[d]);
    }
    TTS_CHECK(ok, TTS_ERR_INVALID, "lstm_backward: every tensor must be 16-byte aligned");
    const int64_t G = 4 * (int64_t)H, BT = (int64_t)B * Tmax, nstate = (int64_t)D * B * H;
    int total = 0, Lmax = 0;
    for (int b = 0; b < B; ++b) {
        Lmax = std::max(Lmax, (int)lens[b]);
        total += lens[b];
    }
    const int nsplit = (total + LT_KC - 1) / LT_KC;
    const int64_t ldg = D * G;
    TTS_TRY(l->dG.reserve((size_t)(BT * ldg)));
    TTS_TRY(l->state.reserve((size_t)(3 * nstate)));
    TTS_TRY(l->partial.reserve((size_t)nsplit * (size_t)(D * G) * (size_t)std::max(I, H)));
    TTS_TRY(stage_maps(l, lens, B, Tmax, &total, s));
    const int* dlens = l->meta.p;
    const int* rowmap = l->meta.p + 2 * B + 1;
    const int* prev[2] = {rowmap + BT, rowmap + 2 * BT};
    const float* rg = reserve;
    const float* rc = reserve + BT * D * H * 4;
    const float* c0copy = reserve + BT * D * H * 5;

    BwdArgs bw{l->whh_t.p, rg, rc, c0copy, grad_out, l->dG.p, l->state.p + nstate, dlens, B, Tmax, H, D, 0};
    const int bt = step_batch_tiles(D * H / 16, B, LT_BWD_BT);
    const dim3 grid((unsigned)(D * H / 16), (unsigned)((B + 16 * bt - 1) / (16 * bt)));
    const auto step_kernel = bt == 1 ? lt_bwd_step_kernel<1> : lt_bwd_step_kernel<LT_BWD_BT>;
    for (int q = 0; q < Lmax; ++q) {
        bw.q = q;
        hipLaunchKernelGGL(step_kernel, grid, dim3(LT_BWD_WAVES * 64), 0, s, bw);
    }
    TTS_HIP(hipGetLastError());

    const int DG = (int)(D * G);
    if (gbi[0] || gbh[0] || gbi[1] || gbh[1]) {
        hipLaunchKernelGGL(lt_colsum_partial_kernel, dim3((unsigned)((DG + 63) / 64), (unsigned)nsplit), dim3(256), 0, s,
                           l->dG.p, ldg, rowmap, total, DG, l->partial.p);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(l->partial.p, nsplit, DG, G, gbi[0], gbi[1], gbh[0], gbh[1], s));
    }
    if (gwi[0] || gwi[1]) {
        const TnArgs t{l->dG.p, ldg, 0, rowmap, x, I, 0, rowmap, nullptr, 0, l->partial.p, DG, I, total};
        hipLaunchKernelGGL(lt_tn_partial_kernel, dim3((unsigned)((I + 63) / 64), (unsigned)(DG / 64), (unsigned)nsplit),
                           dim3(64), 0, s, t);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(l->partial.p, nsplit, (int64_t)DG * I, G * I, gwi[0], gwi[1], nullptr, nullptr, s));
    }
    for (int d = 0; d < D; ++d) {
        if (!gwh[d]) continue;
        const TnArgs t{l->dG.p, ldg, (int)(d * G), rowmap, out, (int64_t)D * H, d * H, prev[d],
                       h0 ? h0 + (int64_t)d * B * H : nullptr, H, l->partial.p, (int)G, H, total};
        hipLaunchKernelGGL(lt_tn_partial_kernel, dim3((unsigned)((H + 63) / 64), (unsigned)(G / 64), (unsigned)nsplit),
                           dim3(64), 0, s, t);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(l->partial.p, nsplit, G * H, G * H, gwh[d], nullptr, nullptr, nullptr, s));
    }
    if (grad_x) {
        hipLaunchKernelGGL(lt_zero_pad_kernel, dim3((unsigned)BT), dim3(64), 0, s, grad_x, I, dlens, Tmax);
        TTS_HIP(hipGetLastError());
        const NtArgs g{l->dG.p, ldg, rowmap, l->wih_t.p, ldg, nullptr, grad_x, I, total, I, DG};
        hipLaunchKernelGGL(lt_nt_gemm_kernel, dim3((unsigned)((g.N + 127) / 128), (unsigned)((g.M + 63) / 64)), dim3(256),
                           0, s, g);
        TTS_HIP(hipGetLastError());
    }
    return TTS_OK;
}

}  // extern "C"
