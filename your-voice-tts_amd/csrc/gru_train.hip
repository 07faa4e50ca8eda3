// Trainable single-layer GRU (one or two directions, every sentence at full length): forward that keeps what
// the backward needs, the backward through time, and the weight / bias / input gradients.  The reference runs
// it as the CBHG's nn.GRU(128, 128, 1, batch_first=True, bidirectional=True) of the encoder and the postnet
// (layers/tacotron.py:165-170, :204-205) and as the GST reference encoder's nn.GRU(256, 128, batch_first=True)
// (layers/gst_layers.py:53-56, :74-78), whose h_n alone is differentiated.
//
// All arithmetic is fp32; every matrix product goes through v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain in
// a fixed k order: within a 16-k chunk k = 4g + j, the four g inside one MFMA, j over four MFMAs); every
// reduction has a fixed order and there are no floating-point atomics, so two runs on the same operands give
// the same bits.
//
// The recurrence is one launch per call.  A workgroup takes one direction and 16 sentences and walks all T
// steps; H / 16 waves, wave w owning units 16w .. 16w + 15.
//   forward:  the wave's rows of W_hh in the three gates (3 x H / 4 registers per lane, MFMA A operands) stay
//             in registers; h_prev of the 16 sentences sits in LDS in MFMA fragment order, double-buffered;
//             xi of the next step is loaded while this step's products run; the cell is the wave's epilogue
//             (MFMA output lane = 4 units of one sentence, the same lane every step, so h_prev of the z * h_prev
//             term is a register).  One workgroup barrier per step.
//   backward: the same with W_hh^T: the wave's 16 columns of dpre_h W_hh over K = 3H (3H / 4 registers), the
//             previous step's dpre_h tile in LDS, dh * z carried in the lane's registers.
// No workgroup waits for another.  Everything that does not feed the recurrence runs as products over all
// B * T rows: xi = x W_ih^T + b_ih (+ b_hh in the r and z rows; b_hh_n starts the hh_n accumulator) before the
// loop; after it the bias gradients (column sums of dpre_i / dpre_h), grad_W_ih = dpre_i^T x and
// grad_W_hh = dpre_h^T h_prev (reduced over the rows in chunks of GT_KC, one partial per chunk, folded in chunk
// order) and grad_x = dpre_i W_ih.  dpre_i = [da_r | da_z | da_n] and dpre_h = [da_r | da_z | da_n * r] differ
// in the n columns only; both are kept.
//
// TTS_GRU_STEPWISE=1 (a diagnostic switch read once, at tts_gru_create; tools/bench_gru_train.py's comparison)
// makes the handle run the same two kernels once per time step, the state travelling through out / dpre_h / a carry buffer instead of LDS and registers.
#include <algorithm>

#include "host_util.h"

namespace tts {
namespace {

typedef float float4a __attribute__((ext_vector_type(4)));

constexpr int GT_KC = 512;   // rows per reduction chunk of the weight gradients
constexpr int GT_MAXH = 128; // a direction's W_hh (3H x H fp32) has to fit one workgroup's registers
constexpr int GT_NT = GT_MAXH / 16;  // most waves of a loop workgroup = most 16-k chunks of H
constexpr int GT_TU = 8;     // groups of 4 rows per load group of gt_tn_partial_kernel

__device__ __forceinline__ float4a ldg4(const float* p) { return *reinterpret_cast<const float4a*>(p); }
__device__ __forceinline__ void stg4(float* p, float4a v) { *reinterpret_cast<float4a*>(p) = v; }

// ------------------------------------------------------------------ weights
// From nn.GRU's layout (w_ih [3H][I], w_hh [3H][H], biases [3H]; gate rows r, z, n) of direction d:
//   whh   [D][3H][H]    as given (the forward recurrence)
//   whh_t [D][H][3H]    transposed (the backward recurrence)
//   wih   [D * 3H][I]   both directions stacked (xi, one GEMM)
//   wih_t [I][D * 3H]   its transpose (grad_x)
//   bias  [D * 3H]      b_ih, plus b_hh in the r and z rows
//   bhn   [D][H]        b_hh of the n rows
struct PackArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float *whh, *whh_t, *wih, *wih_t, *bias, *bhn;
    int I, H, D, d;
};
__global__ void gt_pack_kernel(const PackArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int G = 3 * a.H;
    if (i < (int64_t)G * a.H) {
        const int n = (int)(i / a.H), k = (int)(i - (int64_t)n * a.H);
        const float v = a.w_hh[i];
        a.whh[(int64_t)a.d * G * a.H + i] = v;
        a.whh_t[((int64_t)a.d * a.H + k) * G + n] = v;
    }
    if (i < (int64_t)G * a.I) {
        const int n = (int)(i / a.I), k = (int)(i - (int64_t)n * a.I);
        const float v = a.w_ih[i];
        a.wih[((int64_t)a.d * G + n) * a.I + k] = v;
        a.wih_t[(int64_t)k * a.D * G + a.d * G + n] = v;
    }
    if (i < G) {
        a.bias[a.d * G + i] = i < 2 * a.H ? a.b_ih[i] + a.b_hh[i] : a.b_ih[i];
        if (i >= 2 * a.H) a.bhn[a.d * a.H + (i - 2 * a.H)] = a.b_hh[i];
    }
}

// ------------------------------------------------------------------ C = A W^T (+ bias)
// C[r][n] = sum_k A[r][k] W[n][k] + bias[n], r < M.  K a multiple of 16, N of 16.  A workgroup of four waves
// takes 64 rows x 128 columns, a wave 32 x 64 (2 x 4 MFMA tiles); the next 16 k's operands are loaded before
// the current chunk's MFMAs.
struct NtArgs {
    const float* A;
    int64_t lda;
    const float* W;
    int64_t ldw;
    const float* bias;
    float* C;
    int64_t ldc;
    int M, N, K;
};
__global__ __launch_bounds__(256) void gt_nt_gemm_kernel(const NtArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 64 + (wave & 1) * 32, n0 = blockIdx.y * 128 + (wave >> 1) * 64;  // rows on grid.x
    if (m0 >= a.M || n0 >= a.N) return;  // (wave-uniform; no barrier below)
    const int kq = (lane >> 4) * 4;
    const float* ap[2];
    const float* wp[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int r = m0 + mt * 16 + (lane & 15);
        ap[mt] = r < a.M ? a.A + (int64_t)r * a.lda + kq : nullptr;
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
            float* c = a.C + (int64_t)row * a.ldc;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = n0 + nt * 16 + (lane & 15);
                if (n < a.N) c[n] = acc[mt][nt][r] + (a.bias ? a.bias[n] : 0.f);
            }
        }
}

// ------------------------------------------------------------------ the recurrence
// Fragment order.  MFMA A = 16 weight rows (lane l: row l & 15, k = 4 (l >> 4) + j of a 16-k chunk, j the
// component of a 16-byte load), B = 16 sentences (lane l: sentence l & 15, the same k); the result leaves
// lane l with rows 4 (l >> 4) + 0..3 of sentence l & 15.  So the four values a lane produces for chunk `wave`
// are exactly the 16 bytes lane l reads as B operand of that chunk: a state tile in LDS is [chunk][lane] of 16
// bytes, written and read by lane index, free of bank conflicts.
struct FwdArgs {
    const float* whh;  // [D][3H][H]
    const float* bhn;  // [D][H]
    const float* xi;   // [B][T][D * 3H]
    const float* h0;   // [D][B][H] or null
    float* out;        // [B][T][D * H]
    float* h_n;        // [D][B][H] or null
    float* rs;         // [B][T][D][4][H]: r, z, n, hh_n; or null
    int B, T, H, D, s0, s1;
};

// Steps s0 .. s1 - 1 of direction blockIdx.y (position s forward, T - 1 - s reverse) for sentences
// 16 blockIdx.x ...  blockDim.x = 64 * H / 16.  With s0 > 0 the state is read back from `out`.
__global__ __launch_bounds__(GT_NT * 64) void gt_fwd_loop_kernel(const FwdArgs a) {
    __shared__ float4a hbuf[2][GT_NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, G = 3 * H, nt = H / 16;
    const int d = blockIdx.y, b = blockIdx.x * 16 + (lane & 15), q4 = (lane >> 4) * 4;
    const bool live = b < a.B;  // a lane past the batch loads and stores nothing; its column stays its own
    const int u0 = wave * 16 + q4;
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    float4a w[3][GT_NT];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < GT_NT; ++c) {
            w[g][c] = zero;
            if (c < nt) w[g][c] = ldg4(a.whh + ((int64_t)d * G + g * H + wave * 16 + (lane & 15)) * H + c * 16 + q4);
        }
    const float4a bn = ldg4(a.bhn + d * H + u0);
    const int64_t ldx = (int64_t)a.D * G, row0 = (int64_t)(live ? b : 0) * a.T;
    const int64_t st = ((int64_t)d * a.B + (live ? b : 0)) * H + u0;
    float4a hp = zero;
    if (live) {
        if (a.s0 > 0)
            hp = ldg4(a.out + ((row0 + (d ? a.T - a.s0 : a.s0 - 1)) * a.D + d) * H + u0);
        else if (a.h0)
            hp = ldg4(a.h0 + st);
    }
    hbuf[a.s0 & 1][wave * 64 + lane] = hp;
    float4a xn[3] = {zero, zero, zero};
    if (live) {
        const float* p = a.xi + (row0 + (d ? a.T - 1 - a.s0 : a.s0)) * ldx + d * G + u0;
#pragma unroll
        for (int g = 0; g < 3; ++g) xn[g] = ldg4(p + g * H);
    }
    __syncthreads();
    for (int s = a.s0; s < a.s1; ++s) {
        const int cur = s & 1, t = d ? a.T - 1 - s : s;
        float4a xc[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) xc[g] = xn[g];
        if (s + 1 < a.s1 && live) {  // the next step's xi travels while this step's products run
            const float* p = a.xi + (row0 + (d ? t - 1 : t + 1)) * ldx + d * G + u0;
#pragma unroll
            for (int g = 0; g < 3; ++g) xn[g] = ldg4(p + g * H);
        }
        float4a hv[GT_NT];
#pragma unroll
        for (int c = 0; c < GT_NT; ++c) {
            hv[c] = zero;
            if (c < nt) hv[c] = hbuf[cur][c * 64 + lane];
        }
        floatx4 ar = zero, az = zero, an = bn;
#pragma unroll
        for (int c = 0; c < GT_NT; ++c) {
            if (c >= nt) continue;  // (uniform)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ar = mfma16x16x4(w[0][c][j], hv[c][j], ar);
                az = mfma16x16x4(w[1][c][j], hv[c][j], az);
                an = mfma16x16x4(w[2][c][j], hv[c][j], an);
            }
        }
        float4a rg, zg, ng, hn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rg[r] = sigmoid_cell(xc[0][r] + ar[r]);
            zg[r] = sigmoid_cell(xc[1][r] + az[r]);
            ng[r] = tanh_cell(xc[2][r] + rg[r] * an[r]);
            hn[r] = (1.f - zg[r]) * ng[r] + zg[r] * hp[r];
        }
        hbuf[cur ^ 1][wave * 64 + lane] = hn;
        hp = hn;
        if (live) {
            const int64_t e = (row0 + t) * a.D + d;
            stg4(a.out + e * H + u0, hn);
            if (a.rs) {
                float* p = a.rs + e * 4 * H + u0;
                stg4(p, rg);
                stg4(p + H, zg);
                stg4(p + 2 * H, ng);
                stg4(p + 3 * H, an);
            }
            if (s == a.T - 1 && a.h_n) stg4(a.h_n + st, hn);
        }
        __syncthreads();  // hbuf[cur ^ 1] complete; hbuf[cur] is next written after the next barrier's readers
    }
}

struct BwdArgs {
    const float* whh_t;  // [D][H][3H]
    const float* rs;     // [B][T][D][4][H]
    const float* out;    // [B][T][D * H]
    const float* h0;     // [D][B][H] or null
    const float* gout;   // [B][T][D * H] or null
    const float* ghn;    // [D][B][H] or null
    float* dGi;          // [B][T][D * 3H]
    float* dGh;          // [B][T][D * 3H]
    float* carry;        // [D][B][H] dh * z between stepwise launches, or null
    int B, T, H, D, q0, q1;
};

struct BwdLoads {
    float4a go, rg, zg, ng, hh, hp;
};

// Steps q0 .. q1 - 1 of the backward walk of direction blockIdx.y (position T - 1 - q forward, q reverse).
__global__ __launch_bounds__(GT_NT * 64) void gt_bwd_loop_kernel(const BwdArgs a) {
    __shared__ float4a dbuf[2][3 * GT_NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, G = 3 * H, nt = H / 16;
    const int d = blockIdx.y, b = blockIdx.x * 16 + (lane & 15), q4 = (lane >> 4) * 4;
    const bool live = b < a.B;
    const int u0 = wave * 16 + q4;
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    // k = g * H + c * 16 + ...: chunk g * nt + c of the 3H / 16
    float4a w[3][GT_NT];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < GT_NT; ++c) {
            w[g][c] = zero;
            if (c < nt) w[g][c] = ldg4(a.whh_t + ((int64_t)d * H + wave * 16 + (lane & 15)) * G + g * H + c * 16 + q4);
        }
    const int64_t ldx = (int64_t)a.D * G, row0 = (int64_t)(live ? b : 0) * a.T;
    const int64_t st = ((int64_t)d * a.B + (live ? b : 0)) * H + u0;
    float4a cr = zero;  // dh * z of the step before; the gradient of h_n at the first
    if (live) {
        if (a.q0 > 0)
            cr = ldg4(a.carry + st);
        else if (a.ghn)
            cr = ldg4(a.ghn + st);
    }
    if (a.q0 > 0) {  // a stepwise launch: the previous step's dpre_h comes back from dGh
        const float* p = a.dGh + (row0 + (d ? a.q0 - 1 : a.T - a.q0)) * ldx + d * G + u0;
#pragma unroll
        for (int g = 0; g < 3; ++g) dbuf[a.q0 & 1][(g * nt + wave) * 64 + lane] = live ? ldg4(p + g * H) : zero;
    }
    auto load = [&](int q) {
        BwdLoads v{zero, zero, zero, zero, zero, zero};
        if (!live) return v;
        const int t = d ? q : a.T - 1 - q;
        const int64_t e = (row0 + t) * a.D + d;
        if (a.gout) v.go = ldg4(a.gout + e * H + u0);
        const float* p = a.rs + e * 4 * H + u0;
        v.rg = ldg4(p);
        v.zg = ldg4(p + H);
        v.ng = ldg4(p + 2 * H);
        v.hh = ldg4(p + 3 * H);
        if (q < a.T - 1)
            v.hp = ldg4(a.out + ((row0 + (d ? t + 1 : t - 1)) * a.D + d) * H + u0);
        else if (a.h0)
            v.hp = ldg4(a.h0 + st);
        return v;
    };
    BwdLoads nx = load(a.q0);
    __syncthreads();
    for (int q = a.q0; q < a.q1; ++q) {
        const int cur = q & 1, t = d ? q : a.T - 1 - q;
        const BwdLoads v = nx;
        if (q + 1 < a.q1) nx = load(q + 1);
        floatx4 rec = zero;
        if (q > 0) {
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                float4a dv[GT_NT];
#pragma unroll
                for (int c = 0; c < GT_NT; ++c) {
                    dv[c] = zero;
                    if (c < nt) dv[c] = dbuf[cur][(g * nt + c) * 64 + lane];
                }
#pragma unroll
                for (int c = 0; c < GT_NT; ++c) {
                    if (c >= nt) continue;  // (uniform)
#pragma unroll
                    for (int j = 0; j < 4; ++j) rec = mfma16x16x4(w[g][c][j], dv[c][j], rec);
                }
            }
        }
        float4a dar, daz, dan, dnh;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dh = (v.go[r] + cr[r]) + rec[r];
            const float z = v.zg[r], n = v.ng[r], rg = v.rg[r];
            dan[r] = dh * (1.f - z) * (1.f - n * n);
            daz[r] = dh * (v.hp[r] - n) * z * (1.f - z);
            dar[r] = dan[r] * v.hh[r] * rg * (1.f - rg);
            dnh[r] = dan[r] * rg;
            cr[r] = dh * z;
        }
        dbuf[cur ^ 1][wave * 64 + lane] = dar;
        dbuf[cur ^ 1][(nt + wave) * 64 + lane] = daz;
        dbuf[cur ^ 1][(2 * nt + wave) * 64 + lane] = dnh;
        if (live) {
            float* pi = a.dGi + (row0 + t) * ldx + d * G + u0;
            float* ph = a.dGh + (row0 + t) * ldx + d * G + u0;
            stg4(pi, dar);
            stg4(pi + H, daz);
            stg4(pi + 2 * H, dan);
            stg4(ph, dar);
            stg4(ph + H, daz);
            stg4(ph + 2 * H, dnh);
        }
        __syncthreads();
    }
    if (a.carry && live) stg4(a.carry + st, cr);
}

// ------------------------------------------------------------------ A^T B over the rows
// P[split][m][n] = sum over the chunk's rows r = b * T + t of A[r][acol0 + m] * Bm[r + shift][bcol0 + n].  With
// shift != 0 (grad_W_hh: Bm = out, the direction's previous position) the rows with t == tfirst take row b of
// B0 instead (the initial state; zeros when B0 is null).  One wave per 64 x 64 tile and chunk; per 4 rows a lane
// loads 16 bytes of each operand: component jm of A is column m0 + 4 (l & 15) + jm, i.e. the 64 columns form 4
// interleaved MFMA tiles, the same on the B side, so a lane's four results along n are adjacent.
struct TnArgs {
    const float* A;
    int64_t lda;
    int acol0;
    const float* Bm;
    int64_t ldb;
    int bcol0;
    int shift, tfirst, T;
    const float* B0;
    int64_t ldb0;
    float* P;
    int M, N, K;
};
__global__ __launch_bounds__(64) void gt_tn_partial_kernel(const TnArgs a) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, split = blockIdx.z;
    const int am = m0 + 4 * (lane & 15), bn = n0 + 4 * (lane & 15), kl = lane >> 4;
    const bool mok = am < a.M, nok = bn < a.N;  // M, N multiples of 4
    floatx4 acc[4][4];
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    const int k1 = min(a.K, (split + 1) * GT_KC);
    for (int k0 = split * GT_KC; k0 < k1; k0 += 4 * GT_TU) {
        float4a av[GT_TU], bv[GT_TU];
#pragma unroll
        for (int u = 0; u < GT_TU; ++u) {
            const int r = k0 + 4 * u + kl;
            av[u] = bv[u] = zero;
            if (r >= k1) continue;
            if (mok) av[u] = ldg4(a.A + (int64_t)r * a.lda + a.acol0 + am);
            if (!nok) continue;
            const int b = r / a.T, t = r - b * a.T;
            if (a.shift == 0 || t != a.tfirst)
                bv[u] = ldg4(a.Bm + (int64_t)(r + a.shift) * a.ldb + a.bcol0 + bn);
            else if (a.B0)
                bv[u] = ldg4(a.B0 + (int64_t)b * a.ldb0 + bn);
        }
        __builtin_amdgcn_sched_barrier(0);  // the loads stay together, ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < GT_TU; ++u)
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
            const int m = m0 + 4 * ((lane >> 4) * 4 + r) + jm;
            if (m < a.M)
                stg4(p + (int64_t)m * a.N + bn, float4a{acc[jm][0][r], acc[jm][1][r], acc[jm][2][r], acc[jm][3][r]});
        }
}

// Column sums of dG over a chunk's rows: P[split][n].  A workgroup takes 64 columns; wave w sums the chunk's
// rows w, w + 4, ... in order (8 loads in flight), the waves are folded in index order.
__global__ __launch_bounds__(256) void gt_colsum_partial_kernel(const float* dG, int64_t ld, int K, int N, float* P) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane, split = blockIdx.y;
    const int k1 = min(K, (split + 1) * GT_KC);
    float s = 0.f;
    if (n < N) {
        for (int r0 = split * GT_KC + wave; r0 < k1; r0 += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = r0 + 4 * u;
                v[u] = r < k1 ? dG[(int64_t)r * ld + n] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && n < N) P[(int64_t)split * N + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// dst[e] = P[0][e] + P[1][e] + ... in chunk order; elements [0, half) go to out0, the rest to out1; a null
// destination is skipped.  total, half multiples of 4.
struct FoldArgs {
    const float* P;
    int nsplit;
    int64_t total, half;
    float *out0, *out1;
};
__global__ void gt_fold_kernel(const FoldArgs a) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e >= a.total) return;
    float4a s = ldg4(a.P + e);
    for (int k = 1; k < a.nsplit; ++k) s += ldg4(a.P + k * a.total + e);
    const bool lo = e < a.half;
    float* o = lo ? a.out0 : a.out1;
    if (o) stg4(o + (lo ? e : e - a.half), s);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace tts

struct tts_gru {
    int I = 0, H = 0, D = 0;
    bool have_weights = false;
    bool stepwise = false;  // TTS_GRU_STEPWISE at create
    tts::DeviceBuf<float> whh, whh_t, wih, wih_t, bias, bhn;
    tts::DeviceBuf<float> xi, dGi, dGh, partial, carry;
};

namespace tts {
namespace {

tts_status check_batch(const tts_gru* g, const void* x, int B, int T, const char* what) {
    TTS_CHECK(g && x, TTS_ERR_INVALID, std::string(what) + ": null argument");
    TTS_CHECK(g->have_weights, TTS_ERR_INVALID, std::string(what) + ": tts_gru_set_weights has not been called");
    TTS_CHECK(B > 0 && T > 0, TTS_ERR_INVALID, std::string(what) + ": B and T must be positive");
    TTS_CHECK((int64_t)B * T < (1 << 24), TTS_ERR_INVALID, std::string(what) + ": B * T must be below 2^24");
    return TTS_OK;
}

tts_status fold(const float* P, int nsplit, int64_t total, int64_t half, float* out0, float* out1, hipStream_t s) {
    const FoldArgs f{P, nsplit, total, half, out0, out1};
    hipLaunchKernelGGL(gt_fold_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, f);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_gru_create(int input_size, int hidden_size, int bidirectional, tts_gru** out) {
    TTS_CHECK(out, TTS_ERR_INVALID, "gru_create: null argument");
    TTS_CHECK(input_size > 0 && input_size % 16 == 0, TTS_ERR_UNSUPPORTED,
              "gru_create: input_size must be a positive multiple of 16");
    TTS_CHECK(hidden_size > 0 && hidden_size % 16 == 0 && hidden_size <= GT_MAXH, TTS_ERR_UNSUPPORTED,
              "gru_create: hidden_size must be a positive multiple of 16 that is <= 128");
    tts_gru* g = new tts_gru();
    g->I = input_size;
    g->H = hidden_size;
    g->D = bidirectional ? 2 : 1;
    g->stepwise = env_is("TTS_GRU_STEPWISE", '1');
    *out = g;
    return TTS_OK;
}

void tts_gru_destroy(tts_gru* g) {
    if (!g) return;
    for (float* p : {g->whh.p, g->whh_t.p, g->wih.p, g->wih_t.p, g->bias.p, g->bhn.p, g->xi.p, g->dGi.p, g->dGh.p,
                     g->partial.p, g->carry.p})
        if (p) (void)hipFree(p);
    delete g;
}

tts_status tts_gru_set_weights(tts_gru* g, const float* const* w_ih, const float* const* w_hh,
                               const float* const* b_ih, const float* const* b_hh, void* stream) {
    TTS_CHECK(g && w_ih && w_hh && b_ih && b_hh, TTS_ERR_INVALID, "gru_set_weights: null argument");
    for (int d = 0; d < g->D; ++d)
        TTS_CHECK(w_ih[d] && w_hh[d] && b_ih[d] && b_hh[d], TTS_ERR_INVALID, "gru_set_weights: null tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t G = 3 * (int64_t)g->H;
    TTS_TRY(g->whh.reserve((size_t)(g->D * G * g->H)));
    TTS_TRY(g->whh_t.reserve((size_t)(g->D * g->H * G)));
    TTS_TRY(g->wih.reserve((size_t)(g->D * G * g->I)));
    TTS_TRY(g->wih_t.reserve((size_t)(g->I * g->D * G)));
    TTS_TRY(g->bias.reserve((size_t)(g->D * G)));
    TTS_TRY(g->bhn.reserve((size_t)(g->D * g->H)));
    const int64_t n = G * std::max(g->I, g->H);
    for (int d = 0; d < g->D; ++d) {
        const PackArgs p{w_ih[d],    w_hh[d],     b_ih[d],   b_hh[d],  g->whh.p, g->whh_t.p, g->wih.p,
                         g->wih_t.p, g->bias.p,   g->bhn.p,  g->I,     g->H,     g->D,       d};
        hipLaunchKernelGGL(gt_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
        TTS_HIP(hipGetLastError());
    }
    g->have_weights = true;
    return TTS_OK;
}

int64_t tts_gru_reserve_floats(const tts_gru* g, int B, int T) {
    if (!g || B <= 0 || T <= 0) return 0;
    return (int64_t)B * T * g->D * g->H * 4;
}

tts_status tts_gru_forward(tts_gru* g, const float* x, int B, int T, const float* h0, float* out, float* h_n,
                           float* reserve, void* stream) {
    TTS_TRY(check_batch(g, x, B, T, "gru_forward"));
    TTS_CHECK(out, TTS_ERR_INVALID, "gru_forward: null out");
    TTS_CHECK(aligned16(x) && aligned16(out) && aligned16(h0) && aligned16(h_n) && aligned16(reserve), TTS_ERR_INVALID,
              "gru_forward: x, out, h0, h_n and reserve must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = g->D, H = g->H, I = g->I;
    const int64_t DG = 3 * (int64_t)H * D, BT = (int64_t)B * T;
    TTS_TRY(g->xi.reserve((size_t)(BT * DG)));
    const NtArgs n{x, I, g->wih.p, I, g->bias.p, g->xi.p, DG, (int)BT, (int)DG, I};
    hipLaunchKernelGGL(gt_nt_gemm_kernel, dim3((unsigned)((n.M + 63) / 64), (unsigned)((n.N + 127) / 128)), dim3(256), 0,
                       s, n);
    TTS_HIP(hipGetLastError());
    FwdArgs f{g->whh.p, g->bhn.p, g->xi.p, h0, out, h_n, reserve, B, T, H, D, 0, T};
    const dim3 grid((unsigned)((B + 15) / 16), (unsigned)D), block((unsigned)(64 * (H / 16)));
    if (g->stepwise) {
        for (int step = 0; step < T; ++step) {
            f.s0 = step;
            f.s1 = step + 1;
            hipLaunchKernelGGL(gt_fwd_loop_kernel, grid, block, 0, s, f);
        }
    } else {
        hipLaunchKernelGGL(gt_fwd_loop_kernel, grid, block, 0, s, f);
    }
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status tts_gru_backward(tts_gru* g, const float* x, int B, int T, const float* reserve, const float* out,
                            const float* h0, const float* grad_out, const float* grad_h_n, float* grad_x,
                            float* const* grad_w_ih, float* const* grad_w_hh, float* const* grad_b_ih,
                            float* const* grad_b_hh, void* stream) {
    TTS_TRY(check_batch(g, x, B, T, "gru_backward"));
    TTS_CHECK(reserve && out, TTS_ERR_INVALID, "gru_backward: null reserve or out");
    TTS_CHECK(grad_out || grad_h_n, TTS_ERR_INVALID, "gru_backward: grad_out and grad_h_n are both null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = g->D, H = g->H, I = g->I;
    float *gwi[2] = {}, *gwh[2] = {}, *gbi[2] = {}, *gbh[2] = {};
    bool ok = aligned16(x) && aligned16(reserve) && aligned16(out) && aligned16(h0) && aligned16(grad_out) &&
              aligned16(grad_h_n) && aligned16(grad_x);
    for (int d = 0; d < D; ++d) {
        gwi[d] = grad_w_ih ? grad_w_ih[d] : nullptr;
        gwh[d] = grad_w_hh ? grad_w_hh[d] : nullptr;
        gbi[d] = grad_b_ih ? grad_b_ih[d] : nullptr;
        gbh[d] = grad_b_hh ? grad_b_hh[d] : nullptr;
        ok = ok && aligned16(gwi[d]) && aligned16(gwh[d]) && aligned16(gbi[d]) && aligned16(gbh[d]);
    }
    TTS_CHECK(ok, TTS_ERR_INVALID, "gru_backward: every tensor must be 16-byte aligned");
    const int64_t G = 3 * (int64_t)H, DG = D * G, BT = (int64_t)B * T;
    const int rows = (int)BT, nsplit = (rows + GT_KC - 1) / GT_KC;
    const bool stepwise = g->stepwise;
    TTS_TRY(g->dGi.reserve((size_t)(BT * DG)));
    TTS_TRY(g->dGh.reserve((size_t)(BT * DG)));
    TTS_TRY(g->partial.reserve((size_t)nsplit * (size_t)DG * (size_t)std::max(I, H)));
    if (stepwise) TTS_TRY(g->carry.reserve((size_t)D * B * H));

    BwdArgs bw{g->whh_t.p, reserve, out, h0, grad_out, grad_h_n, g->dGi.p, g->dGh.p, nullptr, B, T, H, D, 0, T};
    const dim3 grid((unsigned)((B + 15) / 16), (unsigned)D), block((unsigned)(64 * (H / 16)));
    if (stepwise) {
        bw.carry = g->carry.p;
        for (int q = 0; q < T; ++q) {
            bw.q0 = q;
            bw.q1 = q + 1;
            hipLaunchKernelGGL(gt_bwd_loop_kernel, grid, block, 0, s, bw);
        }
    } else {
        hipLaunchKernelGGL(gt_bwd_loop_kernel, grid, block, 0, s, bw);
    }
    TTS_HIP(hipGetLastError());

    const dim3 cs_grid((unsigned)((DG + 63) / 64), (unsigned)nsplit);
    if (gbi[0] || gbi[1]) {
        hipLaunchKernelGGL(gt_colsum_partial_kernel, cs_grid, dim3(256), 0, s, g->dGi.p, DG, rows, (int)DG, g->partial.p);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(g->partial.p, nsplit, DG, G, gbi[0], gbi[1], s));
    }
    if (gbh[0] || gbh[1]) {
        hipLaunchKernelGGL(gt_colsum_partial_kernel, cs_grid, dim3(256), 0, s, g->dGh.p, DG, rows, (int)DG, g->partial.p);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(g->partial.p, nsplit, DG, G, gbh[0], gbh[1], s));
    }
    if (gwi[0] || gwi[1]) {
        const TnArgs t{g->dGi.p, DG, 0, x, I, 0, 0, 0, T, nullptr, 0, g->partial.p, (int)DG, I, rows};
        hipLaunchKernelGGL(gt_tn_partial_kernel,
                           dim3((unsigned)((I + 63) / 64), (unsigned)((DG + 63) / 64), (unsigned)nsplit), dim3(64), 0, s, t);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(g->partial.p, nsplit, DG * I, G * I, gwi[0], gwi[1], s));
    }
    for (int d = 0; d < D; ++d) {
        if (!gwh[d]) continue;
        // h_prev of position t: out at t - 1 (forward) / t + 1 (reverse); the initial state at the direction's first
        const TnArgs t{g->dGh.p, DG, (int)(d * G), out, (int64_t)D * H, d * H, d ? 1 : -1, d ? T - 1 : 0, T,
                       h0 ? h0 + (int64_t)d * B * H : nullptr, H, g->partial.p, (int)G, H, rows};
        hipLaunchKernelGGL(gt_tn_partial_kernel,
                           dim3((unsigned)((H + 63) / 64), (unsigned)((G + 63) / 64), (unsigned)nsplit), dim3(64), 0, s, t);
        TTS_HIP(hipGetLastError());
        TTS_TRY(fold(g->partial.p, nsplit, G * H, G * H, gwh[d], nullptr, s));
    }
    if (grad_x) {
        const NtArgs n{g->dGi.p, DG, g->wih_t.p, DG, nullptr, grad_x, I, rows, I, (int)DG};
        hipLaunchKernelGGL(gt_nt_gemm_kernel, dim3((unsigned)((n.M + 63) / 64), (unsigned)((n.N + 127) / 128)), dim3(256),
                           0, s, n);
        TTS_HIP(hipGetLastError());
    }
    return TTS_OK;
}

}  // extern "C"
