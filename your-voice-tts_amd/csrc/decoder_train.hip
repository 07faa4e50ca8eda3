// Trainable Tacotron2 decoder: the teacher-forced forward of the reference's Decoder (layers/tacotron2.py:97-247,
// attention of layers/common_layers.py:107-256 without location attention / transition agent) that keeps what
// the backward needs, and the whole backward through time.
//
// All arithmetic is fp32; every matrix product goes through v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain in
// k order); every reduction has a fixed order and there are no floating-point atomics, so two runs on the same
// operands and masks give the same bits.  Every dependency of the recurrence is a kernel boundary on the
// caller's stream: no persistent kernel, no polling, no device-wide wait, no host copy.
//
// Rows.  Everything inside is step-major: row t * B + b of an array belongs to step t of sentence b, so a step's
// slice is contiguous.  H_att and H_dec have T + 1 slots (slot 0 is the initial state, slot t + 1 what step t
// left), so "the state before step t" is slot t everywhere, the weight gradients included.  Widths that are no
// GEMM dimension (mel * r, the text length L) are padded to multiples of 16 with zeros inside (MRP, Lp).
//
// Forward.  Before the loop: inputs with the masked rows replaced by +0.0 (select), P = inputs Wp^T, the frames,
// the prenet over all T * B rows, xa = prenet W_ih_att[:, :prenet]^T + b_ih + b_hh.  Per step four launches:
//   1 attention LSTM     pre = xa_t + [ctx_{t-1} | h_att] [W_ih[:, prenet:] | W_hh]^T, cell and dropout in the epilogue
//   2 query              q = Wq h_att
//   3 attention          energies, normalisation, forward attention, context (a workgroup per sentence)
//   4 decoder LSTM       pre = b + [h_att | ctx_t | h_dec] [W_ih | W_hh]^T, cell and dropout in the epilogue
// After the loop: the projection over all rows, the stopnet, the copies into the caller's layouts.
// Backward.  Before the loop: the gradient of the projection's input (with the stopnet's share when it is not
// separate).  Per step five launches, walking t = T - 1 .. 0:
//   1 decoder LSTM back  dh = dh_proj_t + dpre_dec_{t+1} W_hh, the cell's backward in the epilogue -> dpre_dec_t
//   2 its input          [dh_att | dctx] = dpre_dec_t W_ih
//   3 attention back     dctx_t (three sources, fixed order), the attention's backward -> dq_t, de, dP +=, d alpha_{t-1}
//   4 attention LSTM back  dh = dh_att + [dq_t | dpre_att_{t+1}] [Wq^T | W_hh^T]^T, cell's backward -> dpre_att_t
//   5 its context input  dctx carried into step t - 1 = dpre_att_t W_ih[:, prenet:]
// After the loop everything that does not feed the recurrence: every weight gradient (A^T B over all rows in
// chunks of DT_KC rows, one partial per chunk, folded in chunk order), grad_inputs = sum_t alpha_t^T dctx_t + dP Wp,
// the prenet's backward, grad_memories, the three one-row embeddings.
//
// In a step product the K dimension is split over the eight waves of a workgroup by 16-k chunks and folded
// through LDS in wave order; no load sits behind a data-dependent branch (an absent operand is loaded from a
// valid dummy address and replaced by zero).
#include <algorithm>

#include "host_util.h"

namespace tts {
namespace {

typedef float float4a __attribute__((ext_vector_type(4)));

constexpr int DT_NW = 8;    // waves of a step workgroup
constexpr int DT_KU = 4;    // 16-k chunks per load group of a step product
constexpr int DT_KC = 512;  // rows per reduction chunk of the weight gradients
constexpr int DT_TU = 8;    // groups of 4 rows per load group of dt_tn_partial_kernel
constexpr int DT_AT = 256;  // threads of an attention workgroup

__device__ __forceinline__ float4a ldg4(const float* p) { return *reinterpret_cast<const float4a*>(p); }
__device__ __forceinline__ void stg4(float* p, float4a v) { *reinterpret_cast<float4a*>(p) = v; }
inline int pad16(int v) { return (v + 15) / 16 * 16; }

// ------------------------------------------------------------------ small kernels
__global__ void dt_fill_kernel(float* p, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// dst[(r -> row) * ldd + dcol0 + c] = src[r * lds + scol0 + c], r < R, c < C (0 where c >= Csrc: padding).
// mode 0: as is.  mode 1: transposed, dst[c * ldd + dcol0 + r].  mode 2: gate rows r = g * H + u -> u * 4 + g.
struct CopyArgs {
    const float* src;
    int64_t lds;
    int scol0, R, C, Csrc;
    float* dst;
    int64_t ldd;
    int dcol0, mode, H;
};
__global__ void dt_copy2d_kernel(const CopyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.R * a.C) return;
    const int r = (int)(i / a.C), c = (int)(i - (int64_t)r * a.C);
    const float v = c < a.Csrc ? a.src[(int64_t)r * a.lds + a.scol0 + c] : 0.f;
    if (a.mode == 1) {
        a.dst[(int64_t)c * a.ldd + a.dcol0 + r] = v;
    } else {
        const int row = a.mode == 2 ? (r % a.H) * 4 + r / a.H : r;
        a.dst[(int64_t)row * a.ldd + a.dcol0 + c] = v;
    }
}

// dst[i] = a[i] + b[i]
__global__ void dt_add_kernel(float* dst, const float* a, const float* b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = a[i] + b[i];
}

// rows [0, B) of dst [.][W] = src [W] (a one-row embedding broadcast over the batch)
__global__ void dt_bcast_kernel(float* dst, const float* src, int B, int W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * W) dst[i] = src[i % W];
}

// inz[b][l][:] = mask[b][l] ? inputs[b][l][:] : +0.0 (select: a masked row's content never reaches a product)
__global__ void dt_sanitize_kernel(const float* in, const uint8_t* mask, float* out, int64_t rows, int W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * W) return;
    const int64_t row = i / W;
    const bool keep = mask ? mask[row] != 0 : true;
    const float v = in[i];
    out[i] = keep ? v : 0.f;
}

// frames [T * B][MRP]: step 0 the go frame, step t the r frames (t - 1) * r .. of memories [B][T * r][mel]
__global__ void dt_frames_kernel(const float* mem, const float* go, float* fr, int B, int T, int MR, int MRP) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)T * B * MRP) return;
    const int j = (int)(i % MRP);
    const int64_t row = i / MRP;
    const int t = (int)(row / B), b = (int)(row - (int64_t)t * B);
    float v = 0.f;
    if (j < MR) v = t == 0 ? go[j] : mem[((int64_t)b * T + (t - 1)) * MR + j];
    fr[i] = v;
}

// h = m ? relu(z) * scale : 0 in place (m null: every element kept)
__global__ void dt_relu_drop_kernel(float* z, const uint8_t* m, float scale, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = z[i];
    const bool keep = m ? m[i] != 0 : true;
    z[i] = keep ? (v > 0.f ? v : 0.f) * scale : 0.f;
}

// dz = h > 0 ? dh * scale : 0 in place on dh (h is the dropped output: h > 0 <=> pre-activation > 0 and kept)
__global__ void dt_relu_drop_bwd_kernel(float* dh, const float* h, float scale, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dh[i] = h[i] > 0.f ? dh[i] * scale : 0.f;
}

// dst [B][T][W] <- src [T * B][lds] columns [0, W)
__global__ void dt_rows_out_kernel(const float* src, int64_t lds, float* dst, int B, int T, int W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * T * W) return;
    const int j = (int)(i % W);
    const int64_t bt = i / W;
    const int b = (int)(bt / T), t = (int)(bt - (int64_t)b * T);
    dst[i] = src[((int64_t)t * B + b) * lds + j];
}

// wave-wide sum in a fixed order (xor butterfly: every lane ends with the same bits)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum over DT_AT threads in a fixed order; red: DT_AT / 64 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < DT_AT / 64; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < DT_AT / 64; ++w) s = fmaxf(s, red[w]);
    return s;
}

// ------------------------------------------------------------------ the stopnet (one output)
// stop[b][t] = sum_k ws[k] * drop([h_dec | out])[k] + bs; a wave per row, lanes strided over k.
struct StopArgs {
    const float* hdec;  // [T * B][R] (slot t + 1)
    const float* outp;  // [T * B][MRP]
    const float *ws, *bs;
    const uint8_t* ms;  // [T * B][R + MR] or null
    float scale;
    float* stop;  // [B][T]
    int B, T, R, MR, MRP;
};
__global__ __launch_bounds__(256) void dt_stop_kernel(const StopArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)a.T * a.B) return;
    const int K = a.R + a.MR;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float x = k < a.R ? a.hdec[row * a.R + k] : a.outp[row * a.MRP + (k - a.R)];
        const bool keep = a.ms ? a.ms[row * K + k] != 0 : true;
        s += a.ws[k] * (keep ? x * a.scale : 0.f);
    }
    s = wave_sum(s);
    const int t = (int)(row / a.B), b = (int)(row - (int64_t)t * a.B);
    if (lane == 0) a.stop[(int64_t)b * a.T + t] = s + a.bs[0];
}

// P[split][k] = sum over the chunk's rows of dstop[row] * drop(x)[row][k], k < K; k == K: sum of dstop
__global__ __launch_bounds__(256) void dt_stop_wgrad_kernel(const StopArgs a, const float* dstop, float* P) {
    const int K = a.R + a.MR;
    const int k = blockIdx.x * 256 + threadIdx.x, split = blockIdx.y;
    if (k > K) return;
    const int64_t rows = (int64_t)a.T * a.B;
    const int64_t r1 = rows < (int64_t)(split + 1) * DT_KC ? rows : (int64_t)(split + 1) * DT_KC;
    float s = 0.f;
    for (int64_t row = (int64_t)split * DT_KC; row < r1; ++row) {
        const int t = (int)(row / a.B), b = (int)(row - (int64_t)t * a.B);
        const float d = dstop[(int64_t)b * a.T + t];
        float x = 1.f;
        if (k < K) {
            x = k < a.R ? a.hdec[row * a.R + k] : a.outp[row * a.MRP + (k - a.R)];
            const bool keep = a.ms ? a.ms[row * K + k] != 0 : true;
            x = keep ? x * a.scale : 0.f;
        }
        s += d * x;
    }
    P[(int64_t)split * (K + 1) + k] = s;
}

// dout [T * B][MRP] = grad_out [B][T][MR] (0 when null, 0 in the padding) + (joint) dstop * ws[R + j] * drop'
__global__ void dt_dout_kernel(const StopArgs a, const float* gout, const float* dstop, float* dout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.T * a.B * a.MRP) return;
    const int j = (int)(i % a.MRP);
    const int64_t row = i / a.MRP;
    const int t = (int)(row / a.B), b = (int)(row - (int64_t)t * a.B);
    float v = 0.f;
    if (j < a.MR) {
        if (gout) v = gout[((int64_t)b * a.T + t) * a.MR + j];
        if (dstop) {
            const bool keep = a.ms ? a.ms[row * (a.R + a.MR) + a.R + j] != 0 : true;
            v += keep ? dstop[(int64_t)b * a.T + t] * a.ws[a.R + j] * a.scale : 0.f;
        }
    }
    dout[i] = v;
}

// dhc [T * B][ld] columns [0, R) += dstop * ws[u] * drop' (the stopnet's share of dh_dec when it is not separate)
__global__ void dt_dh_stop_kernel(const StopArgs a, const float* dstop, float* dhc, int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.T * a.B * a.R) return;
    const int u = (int)(i % a.R);
    const int64_t row = i / a.R;
    const int t = (int)(row / a.B), b = (int)(row - (int64_t)t * a.B);
    const bool keep = a.ms ? a.ms[row * (a.R + a.MR) + u] != 0 : true;
    dhc[row * ld + u] += keep ? dstop[(int64_t)b * a.T + t] * a.ws[u] * a.scale : 0.f;
}

// ------------------------------------------------------------------ C = [A0 | A1] W^T (+ bias) over all rows
// C[r][n] = sum_k A[r][k] W[n][k] + bias[n], r < M, n < N.  K0, K1 multiples of 16.  A workgroup of four waves
// takes 64 rows x 128 columns, a wave 32 x 64 (2 x 4 MFMA tiles); the next 16 k are loaded before the current
// chunk's MFMAs (csrc/lstm_train.hip's lt_nt_gemm_kernel without the row map, with a second operand segment).
struct NtArgs {
    const float* A0;
    int64_t lda0;
    int K0;
    const float* A1;
    int64_t lda1;
    int K1;
    const float* W;
    int64_t ldw;
    const float* bias;
    float* C;
    int64_t ldc;
    int M, N;
};
__global__ __launch_bounds__(256) void dt_nt_gemm_kernel(const NtArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 64 + (wave & 1) * 32, n0 = blockIdx.x * 128 + (wave >> 1) * 64;
    if (m0 >= a.M || n0 >= a.N) return;  // (wave-uniform; no barrier below)
    const int kq = (lane >> 4) * 4, K = a.K0 + a.K1;
    int64_t arow[2];
    bool aok[2], wok[4];
    const float* wp[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int r = m0 + mt * 16 + (lane & 15);
        aok[mt] = r < a.M;
        arow[mt] = aok[mt] ? r : 0;
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + nt * 16 + (lane & 15);
        wok[nt] = n < a.N;
        wp[nt] = a.W + (int64_t)(wok[nt] ? n : 0) * a.ldw + kq;
    }
    floatx4 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    float4a av[2], wv[4];
    auto load = [&](int k, float4a* an, float4a* wn) {
        const bool s0 = k < a.K0;  // (wave-uniform)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float* p = s0 ? a.A0 + arow[mt] * a.lda0 + k + kq : a.A1 + arow[mt] * a.lda1 + (k - a.K0) + kq;
            an[mt] = ldg4(p);
            an[mt] = aok[mt] ? an[mt] : zero;
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            wn[nt] = ldg4(wp[nt] + k);
            wn[nt] = wok[nt] ? wn[nt] : zero;
        }
    };
    load(0, av, wv);
    for (int k = 0; k < K; k += 16) {
        float4a an[2] = {zero, zero}, wn[4] = {zero, zero, zero, zero};
        if (k + 16 < K) load(k + 16, an, wn);
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

// ------------------------------------------------------------------ A^T B over all rows, in chunks
// P[z][m][n] = sum over the rows r of chunk `split` of A[r][m] * Bm[r][n], z = batch * nsplit + split; batch
// shifts both operands by abatch / bbatch floats.  One wave per 64 x 64 tile and chunk; the 64 columns form 4
// interleaved MFMA tiles on both sides, so a lane's four results along n are adjacent (csrc/lstm_train.hip's
// lt_tn_partial_kernel without the maps, with guards on both edges: M, N multiples of 4).
struct TnArgs {
    const float* A;
    int64_t lda, abatch;
    const float* Bm;
    int64_t ldb, bbatch;
    float* P;
    int M, N, K, nsplit;
};
__global__ __launch_bounds__(64) void dt_tn_partial_kernel(const TnArgs a) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int batch = blockIdx.z / a.nsplit, split = blockIdx.z - batch * a.nsplit;
    const int am = m0 + 4 * (lane & 15), bn = n0 + 4 * (lane & 15), kl = lane >> 4;
    const bool mok = am < a.M, nok = bn < a.N;
    const float* A = a.A + batch * a.abatch + (mok ? am : 0);
    const float* Bm = a.Bm + batch * a.bbatch + (nok ? bn : 0);
    floatx4 acc[4][4];
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    const int k1 = min(a.K, (split + 1) * DT_KC);
    for (int k0 = split * DT_KC; k0 < k1; k0 += 4 * DT_TU) {
        float4a av[DT_TU], bv[DT_TU];
#pragma unroll
        for (int u = 0; u < DT_TU; ++u) {
            const int r = k0 + 4 * u + kl;
            const bool in = r < k1;
            const int64_t rr = in ? r : k0;  // (k0 < k1: a valid row)
            av[u] = ldg4(A + rr * a.lda);
            bv[u] = ldg4(Bm + rr * a.ldb);
            av[u] = in && mok ? av[u] : zero;
            bv[u] = in && nok ? bv[u] : zero;
        }
        __builtin_amdgcn_sched_barrier(0);  // the loads stay together, ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < DT_TU; ++u)
#pragma unroll
            for (int jm = 0; jm < 4; ++jm)
#pragma unroll
                for (int jn = 0; jn < 4; ++jn) acc[jm][jn] = mfma16x16x4(av[u][jm], bv[u][jn], acc[jm][jn]);
    }
    if (!nok) return;
    float* p = a.P + (int64_t)blockIdx.z * a.M * a.N;
#pragma unroll
    for (int jm = 0; jm < 4; ++jm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * ((lane >> 4) * 4 + r) + jm;
            if (m < a.M)
                stg4(p + (int64_t)m * a.N + bn, float4a{acc[jm][0][r], acc[jm][1][r], acc[jm][2][r], acc[jm][3][r]});
        }
}

// dst[batch][m * ldd + col0 + n] = P[batch][0][m][n] + P[batch][1][m][n] + ... in chunk order (+ add[...]), m < Mo,
// n < No <= the partials' M, N.  keep (uint8, per batch and row m) selects +0.0 for a masked row.
struct FoldArgs {
    const float* P;
    int nsplit, M, N, Mo, No, nbatch;
    float* dst;
    int64_t ldd, dbatch;
    int col0;
    const float* add;
    const uint8_t* keep;
};
__global__ void dt_fold_kernel(const FoldArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.nbatch * a.Mo * a.No) return;
    const int n = (int)(i % a.No);
    const int64_t bm = i / a.No;
    const int m = (int)(bm % a.Mo), batch = (int)(bm / a.Mo);
    const float* p = a.P + (int64_t)batch * a.nsplit * a.M * a.N + (int64_t)m * a.N + n;
    float s = p[0];
    for (int k = 1; k < a.nsplit; ++k) s += p[(int64_t)k * a.M * a.N];
    const int64_t o = batch * a.dbatch + (int64_t)m * a.ldd + a.col0 + n;
    if (a.add) s += a.add[o];
    const bool keep = a.keep ? a.keep[(int64_t)batch * a.Mo + m] != 0 : true;
    a.dst[o] = keep ? s : 0.f;
}

// Column sums of X [rows][ld] over a chunk's rows: P[split][n].  Wave w of a workgroup sums the chunk's rows
// w, w + 4, ... in order, the waves are folded in index order.
__global__ __launch_bounds__(256) void dt_colsum_partial_kernel(const float* X, int64_t ld, int K, int N, float* P) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane, split = blockIdx.y;
    const int k1 = min(K, (split + 1) * DT_KC);
    float s = 0.f;
    if (n < N)
        for (int r = split * DT_KC + wave; r < k1; r += 4) s += X[(int64_t)r * ld + n];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && n < N) P[(int64_t)split * N + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// ------------------------------------------------------------------ the step product and its epilogues
enum { EPI_PLAIN = 0, EPI_LSTM_FWD = 1, EPI_LSTM_BWD = 2 };

struct StepArgs {
    const float* W;  // [N][k0 + k1 + k2]
    int64_t ldw;
    int N;
    const float* x[3];  // operand segments, rows b
    int64_t ldx[3];
    int k[3];
    int act;  // bit i: segment i is read (else it counts as zeros)
    int B;
    // EPI_PLAIN: C[b][n] = product (+ bias[n])
    const float* bias;  // PLAIN, LSTM_FWD: [N] in the reference's gate order, or null
    float* C;
    int64_t ldc;
    // LSTM_FWD: W rows are u * 4 + gate.  pre = product + add[b][g * H + u] + bias[g * H + u]
    // LSTM_BWD: W rows are units.         dh  = product + add[b][u]
    const float* add;
    int64_t ldadd;
    int H;
    float* cst;  // FWD: the carried (dropped) cell state [B][H]; BWD: the carried cell gradient; in place
    int first;   // FWD: step 0 (the cell state is 0); BWD: step T - 1 (nothing is carried yet)
    const uint8_t *mh, *mc;  // this step's dropout masks [B][H], or null (nothing dropped)
    float scale;
    float* hout;  // FWD: the dropped h [B][H]
    float* rg;    // activated gates [B][H][4]  (FWD: written; BWD: read)
    float* rc;    // c before dropout [B][H]    (FWD: written; BWD: read)
    const float* cprev;     // BWD: rc of step t - 1, or null at step 0 (the cell state was 0)
    const uint8_t* mcprev;  // BWD: mc of step t - 1, or null
    float* dpre;            // BWD: [B][4H] in the reference's gate order
};

// This wave's share of sum_k W[row][k] X[b][k]: MFMA A = 16 weight rows, B = 16 sentences; lane l ends with rows
// (l >> 4) * 4 + 0..3 of sentence l & 15.
template <int BT>
__device__ __forceinline__ void dt_kdot(const StepArgs& a, const float* wrow, const float* const xr[BT][3],
                                        const bool bok[BT], int wave, int lane, floatx4 acc[BT]) {
    const int kq = (lane >> 4) * 4;
    const int s0 = a.k[0], s1 = a.k[0] + a.k[1];
    const int chunks = (s1 + a.k[2]) / 16;
    const float4a zero = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = wave; c0 < chunks; c0 += DT_NW * DT_KU) {
        float4a w[DT_KU], x[DT_KU][BT];
#pragma unroll
        for (int u = 0; u < DT_KU; ++u) {
            const int c = c0 + u * DT_NW;
            const bool in = c < chunks;  // (wave-uniform)
            const int off = (in ? c : c0) * 16 + kq;
            const int seg = off < s0 ? 0 : off < s1 ? 1 : 2;  // (wave-uniform: segments are multiples of 16)
            const bool on = in && ((a.act >> seg) & 1);
            const int xo = off - (seg == 0 ? 0 : seg == 1 ? s0 : s1);
            w[u] = ldg4(wrow + off);
            w[u] = in ? w[u] : zero;
#pragma unroll
            for (int bt = 0; bt < BT; ++bt) {
                const bool rd = on && bok[bt];
                const float* xp = seg == 0 ? xr[bt][0] : seg == 1 ? xr[bt][1] : xr[bt][2];
                x[u][bt] = ldg4(rd ? xp + xo : wrow + off);
                x[u][bt] = rd ? x[u][bt] : zero;
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // the loads stay together, ahead of the MFMAs: one round trip
#pragma unroll
        for (int u = 0; u < DT_KU; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int bt = 0; bt < BT; ++bt) acc[bt] = mfma16x16x4(w[u][j], x[u][bt][j], acc[bt]);
    }
}

// grid.x = N / 16 (rounded up), grid.y = groups of 16 * BT sentences.  Wave w (< BT) finishes batch tile w.
template <int BT, int EPI>
__global__ __launch_bounds__(DT_NW * 64) void dt_step_kernel(const StepArgs a) {
    __shared__ floatx4 red[DT_NW][BT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, g0 = blockIdx.y * 16 * BT;
    const int wr = min(tile * 16 + (lane & 15), a.N - 1);
    const float* wrow = a.W + (int64_t)wr * a.ldw;
    const float* xr[BT][3];
    bool bok[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) {
        const int b = g0 + bt * 16 + (lane & 15);
        bok[bt] = b < a.B;
#pragma unroll
        for (int s = 0; s < 3; ++s) xr[bt][s] = ((a.act >> s) & 1) && bok[bt] ? a.x[s] + (int64_t)b * a.ldx[s] : wrow;
    }
    floatx4 acc[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) acc[bt] = floatx4{0.f, 0.f, 0.f, 0.f};
    dt_kdot<BT>(a, wrow, xr, bok, wave, lane, acc);
#pragma unroll
    for (int bt = 0; bt < BT; ++bt) red[wave][bt][lane] = acc[bt];
    __syncthreads();
    const int eb = g0 + wave * 16 + (lane & 15);
    if (wave >= BT || eb >= a.B) return;
    floatx4 p = red[0][wave][lane];
#pragma unroll
    for (int w = 1; w < DT_NW; ++w) p += red[w][wave][lane];

    if constexpr (EPI == EPI_PLAIN) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = tile * 16 + (lane >> 4) * 4 + r;
            if (n < a.N) a.C[(int64_t)eb * a.ldc + n] = p[r] + (a.bias ? a.bias[n] : 0.f);
        }
    } else if constexpr (EPI == EPI_LSTM_FWD) {
        const int H = a.H, u = tile * 4 + (lane >> 4);
        const int64_t e = (int64_t)eb * H + u;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            pre[g] = p[g];
            if (a.add) pre[g] += a.add[(int64_t)eb * a.ldadd + g * H + u];
            if (a.bias) pre[g] += a.bias[g * H + u];
        }
        const float cp = a.first ? 0.f : a.cst[e];
        const float ig = sigmoid_cell(pre[0]), fg = sigmoid_cell(pre[1]), gg = tanh_cell(pre[2]), og = sigmoid_cell(pre[3]);
        const float c = fg * cp + ig * gg;
        const float h = og * tanh_cell(c);
        const bool kh = a.mh ? a.mh[e] != 0 : true, kc = a.mc ? a.mc[e] != 0 : true;
        a.cst[e] = kc ? c * a.scale : 0.f;
        a.hout[e] = kh ? h * a.scale : 0.f;
        stg4(a.rg + e * 4, float4a{ig, fg, gg, og});
        a.rc[e] = c;
    } else {
        const int H = a.H, u0 = tile * 16 + (lane >> 4) * 4;
        const int64_t e = (int64_t)eb * H + u0;
        float4a dcn, di, df, dg, dO;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4a g = ldg4(a.rg + (e + r) * 4);  // i, f, g, o
            const float c = a.rc[e + r];
            float cp = 0.f;
            if (a.cprev) {
                const bool kp = a.mcprev ? a.mcprev[e + r] != 0 : true;
                cp = kp ? a.cprev[e + r] * a.scale : 0.f;
            }
            const bool kh = a.mh ? a.mh[e + r] != 0 : true, kc = a.mc ? a.mc[e + r] != 0 : true;
            const float dhd = p[r] + a.add[(int64_t)eb * a.ldadd + u0 + r];
            const float dh = kh ? dhd * a.scale : 0.f;
            const float dcd = a.first ? 0.f : a.cst[e + r];
            const float tc = tanh_cell(c);
            const float dc = (kc ? dcd * a.scale : 0.f) + dh * g[3] * (1.f - tc * tc);
            di[r] = dc * g[2] * (g[0] * (1.f - g[0]));
            df[r] = dc * cp * (g[1] * (1.f - g[1]));
            dg[r] = dc * g[0] * (1.f - g[2] * g[2]);
            dO[r] = dh * tc * (g[3] * (1.f - g[3]));
            dcn[r] = dc * g[1];
        }
        stg4(a.cst + e, dcn);
        float* o = a.dpre + (int64_t)eb * 4 * H + u0;
        stg4(o, di);
        stg4(o + H, df);
        stg4(o + 2 * H, dg);
        stg4(o + 3 * H, dO);
    }
}

// ------------------------------------------------------------------ the attention of one step
struct AttnArgs {
    const float* q;      // [B][A] this step's query
    const float* P;      // [B][L][A] processed inputs (0 on masked rows)
    const float* inz;    // [B][L][E] inputs with +0.0 on masked rows
    const float *v, *bv;
    const uint8_t* mask;  // [B][L] or null
    const float* aprev;  // [B][Lp] alpha of step t - 1, or null at step 0
    float* alpha;        // [B][Lp] this step's alpha (fwd: written; bwd: read)
    float* align;        // fwd: [B][T][L] the caller's alignments, row (b, t)
    float* ctx;          // fwd: [B][E]
    int L, Lp, A, E, T, t, norm, fwd;
    // backward
    const float *dx, *dcc;  // dctx from the decoder LSTM's input [B][lddx]; carried from step t + 1 [B][E] or null
    int64_t lddx;
    float* dctx;    // [B][ldc]: in: the projection's share; out: the total
    int64_t ldc;
    float* dal;     // [B][Lp] carried d alpha: in from step t + 1 (not read when last), out for step t - 1
    int last;
    float* dq;      // [B][A]
    float* dvp;     // [B][A + 16]: this (step, sentence)'s share of grad v, then of grad b_v
    float* dP;      // [B][L][A] accumulated in place over the steps
};

// energies into e[l] (l < Lp; 0 past L), normalised into al[l]; returns S (the sigmoid sum, or the softmax's)
// and leaves sg[l] = sigmoid(e_l) (sigmoid norm).  Waves stride over the positions, lanes over the attention units.
__device__ __forceinline__ float dt_alignment(const AttnArgs& a, int b, float* e, float* sg, float* al, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* q = a.q + (int64_t)b * a.A;
    for (int l = wave; l < a.L; l += DT_AT / 64) {
        const float* p = a.P + ((int64_t)b * a.L + l) * a.A;
        float s = 0.f;
        for (int k = lane; k < a.A; k += 64) s += a.v[k] * tanh_cell(q[k] + p[k]);
        s = wave_sum(s);
        if (lane == 0) e[l] = s + a.bv[0];
    }
    __syncthreads();
    float part = 0.f, mx = -INFINITY;
    if (a.norm == 1) {  // softmax
        for (int l = threadIdx.x; l < a.L; l += DT_AT) {
            const bool ok = a.mask ? a.mask[(int64_t)b * a.L + l] != 0 : true;
            mx = ok ? fmaxf(mx, e[l]) : mx;
        }
        mx = block_max(mx, red);
    }
    for (int l = threadIdx.x; l < a.Lp; l += DT_AT) {
        const bool ok = l < a.L && (a.mask ? a.mask[(int64_t)b * a.L + l] != 0 : true);
        const float x = l < a.L ? e[l] : 0.f;
        const float s = a.norm == 1 ? __builtin_amdgcn_exp2f((x - mx) * 1.4426950408889634f) : sigmoid_cell(x);
        sg[l] = ok ? s : 0.f;
        part += sg[l];
    }
    const float S = block_sum(part, red);
    for (int l = threadIdx.x; l < a.Lp; l += DT_AT) al[l] = sg[l] / S;
    __syncthreads();
    return S;
}

// w_l = 0.5 alpha_{t-1}[l] + 0.5 alpha_{t-1}[l - 1] + 1e-8 (alpha_{-1} = [1, 1e-7, ...])
__device__ __forceinline__ float dt_trans(const AttnArgs& a, int b, int l) {
    float p0, p1;
    if (a.aprev) {
        p0 = a.aprev[(int64_t)b * a.Lp + l];
        p1 = l > 0 ? a.aprev[(int64_t)b * a.Lp + l - 1] : 0.f;
    } else {
        p0 = l == 0 ? 1.f : 1e-7f;
        p1 = l == 0 ? 0.f : l == 1 ? 1.f : 1e-7f;
    }
    return (0.5f * p0 + 0.5f * p1) + 1e-8f;
}

__global__ __launch_bounds__(DT_AT) void dt_attn_fwd_kernel(const AttnArgs a) {
    extern __shared__ float sm[];
    __shared__ float red[DT_AT / 64];
    const int b = blockIdx.x;
    float *e = sm, *sg = sm + a.Lp, *al = sm + 2 * a.Lp;
    dt_alignment(a, b, e, sg, al, red);
    if (a.fwd) {
        float part = 0.f;
        for (int l = threadIdx.x; l < a.Lp; l += DT_AT) {
            const float u = l < a.L ? dt_trans(a, b, l) * al[l] : 0.f;
            sg[l] = u;
            part += u;
        }
        const float S2 = block_sum(part, red);
        for (int l = threadIdx.x; l < a.Lp; l += DT_AT) al[l] = sg[l] / S2;
        __syncthreads();
    }
    for (int l = threadIdx.x; l < a.Lp; l += DT_AT) {
        a.alpha[(int64_t)b * a.Lp + l] = al[l];
        if (l < a.L) a.align[((int64_t)b * a.T + a.t) * a.L + l] = al[l];
    }
    const float* x = a.inz + (int64_t)b * a.L * a.E;
    for (int c = threadIdx.x; c < a.E; c += DT_AT) {
        float s = 0.f;
        int l = 0;
        for (; l + 8 <= a.L; l += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = x[(int64_t)(l + u) * a.E + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += al[l + u] * v[u];
        }
        for (; l < a.L; ++l) s += al[l] * x[(int64_t)l * a.E + c];
        a.ctx[(int64_t)b * a.E + c] = s;
    }
}

// dynamic LDS: e, sg, al, da [Lp] each, dctx [E], part [2][DT_AT]
__global__ __launch_bounds__(DT_AT) void dt_attn_bwd_kernel(const AttnArgs a) {
    extern __shared__ float sm[];
    __shared__ float red[DT_AT / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *e = sm, *sg = sm + a.Lp, *al = sm + 2 * a.Lp, *da = sm + 3 * a.Lp, *dc = sm + 4 * a.Lp, *part = dc + a.E;
    // the context's gradient: the decoder LSTM's input, the projection, the next step's attention LSTM
    for (int c = threadIdx.x; c < a.E; c += DT_AT) {
        float s = a.dx[(int64_t)b * a.lddx + c] + a.dctx[(int64_t)b * a.ldc + c];
        if (a.dcc) s += a.dcc[(int64_t)b * a.E + c];
        dc[c] = s;
        a.dctx[(int64_t)b * a.ldc + c] = s;
    }
    const float S = dt_alignment(a, b, e, sg, al, red);  // (its first barrier also covers dc)
    // d alpha_t[l] = carried + dctx . inputs[l]
    const float* x = a.inz + (int64_t)b * a.L * a.E;
    for (int l = wave; l < a.Lp; l += DT_AT / 64) {
        float s = 0.f;
        if (l < a.L)
            for (int c = lane; c < a.E; c += 64) s += dc[c] * x[(int64_t)l * a.E + c];
        s = wave_sum(s);
        if (lane == 0) da[l] = s + ((a.fwd && !a.last) ? a.dal[(int64_t)b * a.Lp + l] : 0.f);
    }
    __syncthreads();
    if (a.fwd) {
        // alpha = u / S2, u = w * alignment
        float p1 = 0.f, p2 = 0.f;
        for (int l = threadIdx.x; l < a.Lp; l += DT_AT) {
            p1 += l < a.L ? dt_trans(a, b, l) * al[l] : 0.f;
            p2 += da[l] * a.alpha[(int64_t)b * a.Lp + l];
        }
        const float S2 = block_sum(p1, red);
        const float D = block_sum(p2, red);
        for (int l = threadIdx.x; l < a.Lp; l += DT_AT) {
            const float du = (da[l] - D) / S2;
            const float w = l < a.L ? dt_trans(a, b, l) : 0.f;
            e[l] = du * al[l];  // d w_l (e is free now)
            da[l] = du * w;     // d alignment_l
        }
        __syncthreads();
        for (int l = threadIdx.x; l < a.Lp; l += DT_AT)
            a.dal[(int64_t)b * a.Lp + l] = 0.5f * e[l] + 0.5f * (l + 1 < a.Lp ? e[l + 1] : 0.f);
    }
    // alignment = sg / S (sigmoid: sg = sigmoid(e); softmax: sg = exp(e - max))
    float p3 = 0.f;
    for (int l = threadIdx.x; l < a.Lp; l += DT_AT) p3 += da[l] * al[l];
    const float D2 = block_sum(p3, red);
    for (int l = threadIdx.x; l < a.Lp; l += DT_AT) {
        const float ds = (da[l] - D2) / S;
        const float de = a.norm == 1 ? al[l] * (da[l] - D2) : ds * (sg[l] * (1.f - sg[l]));
        const bool ok = l < a.L && (a.mask ? a.mask[(int64_t)b * a.L + l] != 0 : true);
        da[l] = ok ? de : 0.f;  // d e_l
    }
    __syncthreads();
    // dq, dP, v's share: thread (group, k) takes unit k at the positions group, group + ng, ...
    const int ng = max(1, DT_AT / a.A);
    const float* q = a.q + (int64_t)b * a.A;
    for (int k0 = 0; k0 < a.A; k0 += DT_AT) {
        const int grp = a.A >= DT_AT ? 0 : threadIdx.x / a.A;
        const int k = a.A >= DT_AT ? k0 + threadIdx.x : threadIdx.x - grp * a.A;
        float sq = 0.f, sv = 0.f;
        if (grp < ng && k < a.A) {
            const float vk = a.v[k], qk = q[k];
            for (int l = grp; l < a.L; l += ng) {
                const int64_t i = ((int64_t)b * a.L + l) * a.A + k;
                const float th = tanh_cell(qk + a.P[i]);
                const float d = da[l] * vk * (1.f - th * th);
                sq += d;
                sv += da[l] * th;
                a.dP[i] += d;
            }
        }
        __syncthreads();
        part[threadIdx.x] = sq;
        part[DT_AT + threadIdx.x] = sv;
        __syncthreads();
        if (grp == 0 && k < a.A) {
            const int kk = a.A >= DT_AT ? (int)threadIdx.x : k;
            float tq = part[kk], tv = part[DT_AT + kk];
            for (int g = 1; g < ng; ++g) {
                tq += part[g * a.A + kk];
                tv += part[DT_AT + g * a.A + kk];
            }
            a.dq[(int64_t)b * a.A + k] = tq;
            a.dvp[(int64_t)b * (a.A + 16) + k] = tv;
        }
    }
    float p4 = 0.f;
    for (int l = threadIdx.x; l < a.Lp; l += DT_AT) p4 += da[l];
    const float Db = block_sum(p4, red);
    if (threadIdx.x < 16) a.dvp[(int64_t)b * (a.A + 16) + a.A + threadIdx.x] = threadIdx.x == 0 ? Db : 0.f;
}

// grad_memories [B][T * r][mel] from dframes [T * B][MRP]: frame group g feeds step g + 1; the last group feeds none
__global__ void dt_gmem_kernel(const float* dfr, float* gmem, int B, int T, int MR, int MRP) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * T * MR) return;
    const int j = (int)(i % MR);
    const int64_t bg = i / MR;
    const int b = (int)(bg / T), g = (int)(bg - (int64_t)b * T);
    gmem[i] = g + 1 < T ? dfr[((int64_t)(g + 1) * B + b) * MRP + j] : 0.f;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace tts

struct tts_dectrain {
    int E = 0, PN = 0, R = 0, A = 0, MR = 0, MRP = 0;
    int norm = 0, fwd_attn = 0, prenet_dropout = 0, separate = 0;
    bool have_weights = false;
    // repacked weights (one block) and the pointers into it
    tts::DeviceBuf<float> wbuf;
    float *w1 = nullptr, *w1t = nullptr, *w2 = nullptr, *w2t = nullptr;  // prenet [PN][MRP], [MRP][PN], [PN][PN] x 2
    float *wap = nullptr, *wapt = nullptr, *ba = nullptr;                // W_ih_att[:, :PN] [4R][PN], its transpose, b_ih + b_hh
    float *wfa = nullptr, *wfd = nullptr, *bd = nullptr;                 // gate-packed [4R][E + R], [4R][R + E + R], b_ih + b_hh
    float *wq = nullptr, *wp = nullptr, *wpt = nullptr;                  // [A][R], [A][E], [E][A]
    float *wta_h = nullptr, *wta_c = nullptr;                            // [R][A + 4R] = [Wq^T | W_hh_att^T], [E][4R]
    float *wtd_h = nullptr, *wtd_x = nullptr;                            // [R][4R], [R + E][4R]
    float *wproj = nullptr, *wprojt = nullptr, *bproj = nullptr;         // [MR][R + E], [R + E][MRP], [MR]
    float *v = nullptr, *bv = nullptr, *ws = nullptr, *bs = nullptr, *go = nullptr, *ia = nullptr, *id = nullptr;
    tts::DeviceBuf<float> fws, bws, partial;  // the forward's block without a reserve, the backward's, the partials
};

namespace tts {
namespace {

// The reserve: offsets in floats of what a forward keeps.
struct Reserve {
    int64_t hatt, hdec, ctx, alpha, q, gatt, catt, gdec, cdec, h1, h2, fr, outp, P, inz, total;
};
Reserve reserve_layout(const tts_dectrain* h, int B, int L, int T) {
    const int64_t TB = (int64_t)T * B, Lp = pad16(L);
    Reserve r;
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += (n + 3) / 4 * 4;
        return at;
    };
    r.hatt = take((TB + B) * h->R);
    r.hdec = take((TB + B) * h->R);
    r.ctx = take(TB * h->E);
    r.alpha = take(TB * Lp);
    r.q = take(TB * h->A);
    r.gatt = take(TB * h->R * 4);
    r.catt = take(TB * h->R);
    r.gdec = take(TB * h->R * 4);
    r.cdec = take(TB * h->R);
    r.h1 = take(TB * h->PN);
    r.h2 = take(TB * h->PN);
    r.fr = take(TB * h->MRP);
    r.outp = take(TB * h->MRP);
    r.P = take((int64_t)B * L * h->A);
    r.inz = take((int64_t)B * L * h->E);
    r.total = o;
    return r;
}

inline unsigned blocks(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

tts_status nt_gemm(const float* A0, int64_t lda0, int K0, const float* A1, int64_t lda1, int K1, const float* W,
                   int64_t ldw, const float* bias, float* C, int64_t ldc, int64_t M, int N, hipStream_t s) {
    const NtArgs g{A0, lda0, K0, A1, lda1, K1, W, ldw, bias, C, ldc, (int)M, N};
    hipLaunchKernelGGL(dt_nt_gemm_kernel, dim3((unsigned)((N + 127) / 128), (unsigned)((M + 63) / 64)), dim3(256), 0, s, g);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

// dst[m * ldd + col0 + n] (m < Mo, n < No) = sum over K rows of A[r][m] Bm[r][n]
tts_status tn_product(tts_dectrain* h, const float* A, int64_t lda, int M, const float* Bm, int64_t ldb, int N, int64_t K,
                      float* dst, int64_t ldd, int col0, int Mo, int No, hipStream_t s) {
    if (!dst) return TTS_OK;
    const int nsplit = (int)std::max<int64_t>(1, (K + DT_KC - 1) / DT_KC);
    const TnArgs t{A, lda, 0, Bm, ldb, 0, h->partial.p, M, N, (int)K, nsplit};
    hipLaunchKernelGGL(dt_tn_partial_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64), (unsigned)nsplit),
                       dim3(64), 0, s, t);
    TTS_HIP(hipGetLastError());
    const FoldArgs f{h->partial.p, nsplit, M, N, Mo, No, 1, dst, ldd, 0, col0, nullptr, nullptr};
    hipLaunchKernelGGL(dt_fold_kernel, dim3(blocks((int64_t)Mo * No)), dim3(256), 0, s, f);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

// dst[n] (n < No) = sum over K rows of X[r][n]
tts_status col_sum(tts_dectrain* h, const float* X, int64_t ld, int64_t K, int N, float* dst, int No, hipStream_t s) {
    if (!dst) return TTS_OK;
    const int nsplit = (int)std::max<int64_t>(1, (K + DT_KC - 1) / DT_KC);
    hipLaunchKernelGGL(dt_colsum_partial_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)nsplit), dim3(256), 0, s, X, ld,
                       (int)K, N, h->partial.p);
    TTS_HIP(hipGetLastError());
    const FoldArgs f{h->partial.p, nsplit, 1, N, 1, No, 1, dst, No, 0, 0, nullptr, nullptr};
    hipLaunchKernelGGL(dt_fold_kernel, dim3(blocks(No)), dim3(256), 0, s, f);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

template <int EPI>
tts_status step_launch(const StepArgs& a, hipStream_t s) {
    const int bt = a.B > 16 ? 2 : 1;
    const dim3 grid((unsigned)((a.N + 15) / 16), (unsigned)((a.B + 16 * bt - 1) / (16 * bt)));
    if (bt == 2)
        hipLaunchKernelGGL((dt_step_kernel<2, EPI>), grid, dim3(DT_NW * 64), 0, s, a);
    else
        hipLaunchKernelGGL((dt_step_kernel<1, EPI>), grid, dim3(DT_NW * 64), 0, s, a);
    return TTS_OK;
}

tts_status copy2d(const float* src, int64_t lds, int scol0, int R, int C, int Csrc, float* dst, int64_t ldd, int dcol0,
                  int mode, int H, hipStream_t s) {
    const CopyArgs c{src, lds, scol0, R, C, Csrc, dst, ldd, dcol0, mode, H};
    hipLaunchKernelGGL(dt_copy2d_kernel, dim3(blocks((int64_t)R * C)), dim3(256), 0, s, c);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status check_shape(const tts_dectrain* h, int B, int L, int T, const char* what) {
    TTS_CHECK(h, TTS_ERR_INVALID, std::string(what) + ": null handle");
    TTS_CHECK(h->have_weights, TTS_ERR_INVALID, std::string(what) + ": tts_dectrain_set_weights has not been called");
    TTS_CHECK(B > 0 && L > 0 && T > 0, TTS_ERR_INVALID, std::string(what) + ": B, L and T must be positive");
    TTS_CHECK((int64_t)B * T < (1 << 24) && (int64_t)B * L < (1 << 24) && L <= 2048, TTS_ERR_INVALID,
              std::string(what) + ": B * T, B * L or L too large");
    // the attention's backward keeps 4 rows of Lp floats, the context's gradient and two rows of partials in LDS
    TTS_CHECK((size_t)(4 * pad16(L) + h->E + 2 * DT_AT) * sizeof(float) <= 64 * 1024, TTS_ERR_INVALID,
              std::string(what) + ": 4 * L + enc too large for the attention kernels' 64 KB of LDS");
    return TTS_OK;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_dectrain_create(int enc, int prenet, int rnn, int att, int mel_r, int norm, int forward_attn,
                               int prenet_dropout, int separate_stopnet, tts_dectrain** out) {
    TTS_CHECK(out, TTS_ERR_INVALID, "dectrain_create: null argument");
    TTS_CHECK(norm == 0 || norm == 1, TTS_ERR_INVALID, "dectrain_create: norm must be 0 (sigmoid) or 1 (softmax)");
    for (int d : {enc, prenet, rnn, att})
        TTS_CHECK(d > 0 && d % 16 == 0, TTS_ERR_UNSUPPORTED,
                  "dectrain_create: enc, prenet, rnn and att must be positive multiples of 16");
    TTS_CHECK(mel_r > 0, TTS_ERR_UNSUPPORTED, "dectrain_create: mel * r must be positive");
    tts_dectrain* h = new tts_dectrain();
    h->E = enc;
    h->PN = prenet;
    h->R = rnn;
    h->A = att;
    h->MR = mel_r;
    h->MRP = pad16(mel_r);
    h->norm = norm;
    h->fwd_attn = forward_attn != 0;
    h->prenet_dropout = prenet_dropout != 0;
    h->separate = separate_stopnet != 0;
    *out = h;
    return TTS_OK;
}

void tts_dectrain_destroy(tts_dectrain* h) {
    if (!h) return;
    for (float* p : {h->wbuf.p, h->fws.p, h->bws.p, h->partial.p})
        if (p) (void)hipFree(p);
    delete h;
}

tts_status tts_dectrain_set_weights(tts_dectrain* h, const tts_dectrain_weights* w, void* stream) {
    TTS_CHECK(h && w, TTS_ERR_INVALID, "dectrain_set_weights: null argument");
    const float* all[] = {w->prenet_w1, w->prenet_w2, w->att_w_ih, w->att_w_hh, w->att_b_ih, w->att_b_hh, w->query_w,
                          w->inputs_w, w->v_w, w->v_b, w->dec_w_ih, w->dec_w_hh, w->dec_b_ih, w->dec_b_hh, w->proj_w,
                          w->proj_b, w->stop_w, w->stop_b, w->att_init, w->go_init, w->dec_init};
    for (const float* p : all) TTS_CHECK(p, TTS_ERR_INVALID, "dectrain_set_weights: null tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int E = h->E, PN = h->PN, R = h->R, A = h->A, MR = h->MR, MRP = h->MRP, G = 4 * R;
    size_t o = 0;
    auto take = [&](size_t n) {
        const size_t at = o;
        o += (n + 3) / 4 * 4;
        return at;
    };
    const size_t o_w1 = take((size_t)PN * MRP), o_w1t = take((size_t)MRP * PN), o_w2 = take((size_t)PN * PN),
                 o_w2t = take((size_t)PN * PN), o_wap = take((size_t)G * PN), o_wapt = take((size_t)PN * G),
                 o_ba = take(G), o_wfa = take((size_t)G * (E + R)), o_wfd = take((size_t)G * (2 * R + E)), o_bd = take(G),
                 o_wq = take((size_t)A * R), o_wp = take((size_t)A * E), o_wpt = take((size_t)E * A),
                 o_wta_h = take((size_t)R * (A + G)), o_wta_c = take((size_t)E * G), o_wtd_h = take((size_t)R * G),
                 o_wtd_x = take((size_t)(R + E) * G), o_wproj = take((size_t)MRP * (R + E)),
                 o_wprojt = take((size_t)(R + E) * MRP), o_bproj = take(MRP), o_v = take(A), o_bv = take(4),
                 o_ws = take(R + MR), o_bs = take(4), o_go = take(MRP), o_ia = take(R), o_id = take(R);
    TTS_TRY(h->wbuf.reserve(o));
    float* base = h->wbuf.p;
    h->w1 = base + o_w1, h->w1t = base + o_w1t, h->w2 = base + o_w2, h->w2t = base + o_w2t;
    h->wap = base + o_wap, h->wapt = base + o_wapt, h->ba = base + o_ba, h->wfa = base + o_wfa, h->wfd = base + o_wfd;
    h->bd = base + o_bd, h->wq = base + o_wq, h->wp = base + o_wp, h->wpt = base + o_wpt, h->wta_h = base + o_wta_h;
    h->wta_c = base + o_wta_c, h->wtd_h = base + o_wtd_h, h->wtd_x = base + o_wtd_x, h->wproj = base + o_wproj;
    h->wprojt = base + o_wprojt, h->bproj = base + o_bproj, h->v = base + o_v, h->bv = base + o_bv, h->ws = base + o_ws;
    h->bs = base + o_bs, h->go = base + o_go, h->ia = base + o_ia, h->id = base + o_id;
    // prenet: K padded to MRP with zeros
    TTS_TRY(copy2d(w->prenet_w1, MR, 0, PN, MRP, MR, h->w1, MRP, 0, 0, 0, s));
    TTS_TRY(copy2d(w->prenet_w1, MR, 0, PN, MRP, MR, h->w1t, PN, 0, 1, 0, s));
    TTS_TRY(copy2d(w->prenet_w2, PN, 0, PN, PN, PN, h->w2, PN, 0, 0, 0, s));
    TTS_TRY(copy2d(w->prenet_w2, PN, 0, PN, PN, PN, h->w2t, PN, 0, 1, 0, s));
    // attention LSTM: W_ih = [prenet part | context part]
    TTS_TRY(copy2d(w->att_w_ih, PN + E, 0, G, PN, PN, h->wap, PN, 0, 0, 0, s));
    TTS_TRY(copy2d(w->att_w_ih, PN + E, 0, G, PN, PN, h->wapt, G, 0, 1, 0, s));
    TTS_TRY(copy2d(w->att_w_ih, PN + E, PN, G, E, E, h->wfa, E + R, 0, 2, R, s));
    TTS_TRY(copy2d(w->att_w_hh, R, 0, G, R, R, h->wfa, E + R, E, 2, R, s));
    TTS_TRY(copy2d(w->att_w_ih, PN + E, PN, G, E, E, h->wta_c, G, 0, 1, 0, s));
    TTS_TRY(copy2d(w->query_w, R, 0, A, R, R, h->wta_h, A + G, 0, 1, 0, s));
    TTS_TRY(copy2d(w->att_w_hh, R, 0, G, R, R, h->wta_h, A + G, A, 1, 0, s));
    hipLaunchKernelGGL(dt_add_kernel, dim3(blocks(G)), dim3(256), 0, s, h->ba, w->att_b_ih, w->att_b_hh, G);
    // decoder LSTM
    TTS_TRY(copy2d(w->dec_w_ih, R + E, 0, G, R + E, R + E, h->wfd, 2 * R + E, 0, 2, R, s));
    TTS_TRY(copy2d(w->dec_w_hh, R, 0, G, R, R, h->wfd, 2 * R + E, R + E, 2, R, s));
    TTS_TRY(copy2d(w->dec_w_hh, R, 0, G, R, R, h->wtd_h, G, 0, 1, 0, s));
    TTS_TRY(copy2d(w->dec_w_ih, R + E, 0, G, R + E, R + E, h->wtd_x, G, 0, 1, 0, s));
    hipLaunchKernelGGL(dt_add_kernel, dim3(blocks(G)), dim3(256), 0, s, h->bd, w->dec_b_ih, w->dec_b_hh, G);
    // attention, projection, stopnet, the three rows
    TTS_TRY(copy2d(w->query_w, R, 0, A, R, R, h->wq, R, 0, 0, 0, s));
    TTS_TRY(copy2d(w->inputs_w, E, 0, A, E, E, h->wp, E, 0, 0, 0, s));
    TTS_TRY(copy2d(w->inputs_w, E, 0, A, E, E, h->wpt, A, 0, 1, 0, s));
    TTS_TRY(copy2d(w->proj_w, R + E, 0, MR, R + E, R + E, h->wproj, R + E, 0, 0, 0, s));
    hipLaunchKernelGGL(dt_fill_kernel, dim3(blocks((int64_t)(R + E) * MRP)), dim3(256), 0, s, h->wprojt,
                       (int64_t)(R + E) * MRP, 0.f);
    TTS_TRY(copy2d(w->proj_w, R + E, 0, MR, R + E, R + E, h->wprojt, MRP, 0, 1, 0, s));
    TTS_TRY(copy2d(w->proj_b, MR, 0, 1, MR, MR, h->bproj, MRP, 0, 0, 0, s));
    TTS_TRY(copy2d(w->v_w, A, 0, 1, A, A, h->v, A, 0, 0, 0, s));
    TTS_TRY(copy2d(w->v_b, 1, 0, 1, 1, 1, h->bv, 1, 0, 0, 0, s));
    TTS_TRY(copy2d(w->stop_w, R + MR, 0, 1, R + MR, R + MR, h->ws, R + MR, 0, 0, 0, s));
    TTS_TRY(copy2d(w->stop_b, 1, 0, 1, 1, 1, h->bs, 1, 0, 0, 0, s));
    TTS_TRY(copy2d(w->go_init, MR, 0, 1, MRP, MR, h->go, MRP, 0, 0, 0, s));
    TTS_TRY(copy2d(w->att_init, R, 0, 1, R, R, h->ia, R, 0, 0, 0, s));
    TTS_TRY(copy2d(w->dec_init, R, 0, 1, R, R, h->id, R, 0, 0, 0, s));
    TTS_HIP(hipGetLastError());
    h->have_weights = true;
    return TTS_OK;
}

int64_t tts_dectrain_reserve_floats(const tts_dectrain* h, int B, int L, int T) {
    if (!h || B <= 0 || L <= 0 || T <= 0) return 0;
    return reserve_layout(h, B, L, T).total;
}

tts_status tts_dectrain_forward(tts_dectrain* h, const float* inputs, const float* memories, const uint8_t* mask, int B,
                                int L, int T, int training, const tts_dectrain_masks* m, float* out, float* stop,
                                float* alignments, float* reserve, void* stream) {
    TTS_TRY(check_shape(h, B, L, T, "dectrain_forward"));
    TTS_CHECK(inputs && memories && out && stop && alignments, TTS_ERR_INVALID, "dectrain_forward: null tensor");
    TTS_CHECK(aligned16(reserve), TTS_ERR_INVALID, "dectrain_forward: the reserve must be 16-byte aligned");
    const bool tr = training != 0;
    if (tr) {
        TTS_CHECK(m && m->att_h && m->att_c && m->dec_h && m->dec_c && m->stop, TTS_ERR_INVALID,
                  "dectrain_forward: training needs the dropout masks");
        TTS_CHECK(!h->prenet_dropout || (m->prenet1 && m->prenet2), TTS_ERR_INVALID,
                  "dectrain_forward: training with prenet dropout needs the prenet masks");
        TTS_CHECK(m->scale_rnn > 0.f && m->scale_stop > 0.f && (!h->prenet_dropout || m->scale_prenet > 0.f),
                  TTS_ERR_INVALID, "dectrain_forward: the dropout scales must be positive");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int E = h->E, PN = h->PN, R = h->R, A = h->A, MR = h->MR, MRP = h->MRP, G = 4 * R, Lp = pad16(L);
    const int64_t TB = (int64_t)T * B;
    const Reserve lay = reserve_layout(h, B, L, T);
    float* base = reserve;
    if (!base) {
        TTS_TRY(h->fws.reserve((size_t)lay.total));
        base = h->fws.p;
    }
    // per-call workspace: xa [TB][4R], the two carried cell states [B][R]
    TTS_TRY(h->bws.reserve((size_t)(TB * G + 2 * (int64_t)B * R)));
    float *xa = h->bws.p, *catt = xa + TB * G, *cdec = catt + (int64_t)B * R;
    float *hatt = base + lay.hatt, *hdec = base + lay.hdec, *ctx = base + lay.ctx, *alpha = base + lay.alpha;
    float *q = base + lay.q, *h1 = base + lay.h1, *h2 = base + lay.h2, *fr = base + lay.fr, *outp = base + lay.outp;
    float *P = base + lay.P, *inz = base + lay.inz;
    const bool pd = tr && h->prenet_dropout;
    const float srnn = tr ? m->scale_rnn : 1.f;

    hipLaunchKernelGGL(dt_sanitize_kernel, dim3(blocks((int64_t)B * L * E)), dim3(256), 0, s, inputs, mask, inz,
                       (int64_t)B * L, E);
    TTS_TRY(nt_gemm(inz, E, E, nullptr, 0, 0, h->wp, E, nullptr, P, A, (int64_t)B * L, A, s));
    hipLaunchKernelGGL(dt_frames_kernel, dim3(blocks(TB * MRP)), dim3(256), 0, s, memories, h->go, fr, B, T, MR, MRP);
    TTS_TRY(nt_gemm(fr, MRP, MRP, nullptr, 0, 0, h->w1, MRP, nullptr, h1, PN, TB, PN, s));
    hipLaunchKernelGGL(dt_relu_drop_kernel, dim3(blocks(TB * PN)), dim3(256), 0, s, h1, pd ? m->prenet1 : nullptr,
                       pd ? m->scale_prenet : 1.f, TB * PN);
    TTS_TRY(nt_gemm(h1, PN, PN, nullptr, 0, 0, h->w2, PN, nullptr, h2, PN, TB, PN, s));
    hipLaunchKernelGGL(dt_relu_drop_kernel, dim3(blocks(TB * PN)), dim3(256), 0, s, h2, pd ? m->prenet2 : nullptr,
                       pd ? m->scale_prenet : 1.f, TB * PN);
    TTS_TRY(nt_gemm(h2, PN, PN, nullptr, 0, 0, h->wap, PN, h->ba, xa, G, TB, G, s));
    hipLaunchKernelGGL(dt_bcast_kernel, dim3(blocks((int64_t)B * R)), dim3(256), 0, s, hatt, h->ia, B, R);
    hipLaunchKernelGGL(dt_bcast_kernel, dim3(blocks((int64_t)B * R)), dim3(256), 0, s, hdec, h->id, B, R);
    TTS_HIP(hipGetLastError());

    const size_t lds = (size_t)3 * Lp * sizeof(float);
    for (int t = 0; t < T; ++t) {
        const int64_t row = (int64_t)t * B;
        StepArgs a{};
        a.W = h->wfa, a.ldw = E + R, a.N = G, a.B = B, a.H = R;
        a.x[0] = ctx + (row - B) * E, a.ldx[0] = E, a.k[0] = E;
        a.x[1] = hatt + row * R, a.ldx[1] = R, a.k[1] = R;
        a.x[2] = nullptr, a.ldx[2] = 0, a.k[2] = 0;
        a.act = t > 0 ? 3 : 2;
        a.add = xa + row * G, a.ldadd = G, a.bias = nullptr;
        a.cst = catt, a.first = t == 0;
        a.mh = tr ? m->att_h + row * R : nullptr, a.mc = tr ? m->att_c + row * R : nullptr, a.scale = srnn;
        a.hout = hatt + (row + B) * R;
        a.rg = base + lay.gatt + row * R * 4, a.rc = base + lay.catt + row * R;
        TTS_TRY(step_launch<EPI_LSTM_FWD>(a, s));

        StepArgs g{};
        g.W = h->wq, g.ldw = R, g.N = A, g.B = B;
        g.x[0] = hatt + (row + B) * R, g.ldx[0] = R, g.k[0] = R, g.act = 1;
        g.C = q + row * A, g.ldc = A;
        TTS_TRY(step_launch<EPI_PLAIN>(g, s));

        AttnArgs at{};
        at.q = q + row * A, at.P = P, at.inz = inz, at.v = h->v, at.bv = h->bv, at.mask = mask;
        at.aprev = t > 0 ? alpha + (row - B) * Lp : nullptr, at.alpha = alpha + row * Lp, at.align = alignments;
        at.ctx = ctx + row * E;
        at.L = L, at.Lp = Lp, at.A = A, at.E = E, at.T = T, at.t = t, at.norm = h->norm, at.fwd = h->fwd_attn;
        hipLaunchKernelGGL(dt_attn_fwd_kernel, dim3((unsigned)B), dim3(DT_AT), lds, s, at);

        StepArgs d{};
        d.W = h->wfd, d.ldw = 2 * R + E, d.N = G, d.B = B, d.H = R;
        d.x[0] = hatt + (row + B) * R, d.ldx[0] = R, d.k[0] = R;
        d.x[1] = ctx + row * E, d.ldx[1] = E, d.k[1] = E;
        d.x[2] = hdec + row * R, d.ldx[2] = R, d.k[2] = R;
        d.act = 7;
        d.add = nullptr, d.bias = h->bd;
        d.cst = cdec, d.first = t == 0;
        d.mh = tr ? m->dec_h + row * R : nullptr, d.mc = tr ? m->dec_c + row * R : nullptr, d.scale = srnn;
        d.hout = hdec + (row + B) * R;
        d.rg = base + lay.gdec + row * R * 4, d.rc = base + lay.cdec + row * R;
        TTS_TRY(step_launch<EPI_LSTM_FWD>(d, s));
    }
    TTS_HIP(hipGetLastError());

    TTS_TRY(nt_gemm(hdec + (int64_t)B * R, R, R, ctx, E, E, h->wproj, R + E, h->bproj, outp, MRP, TB, MR, s));
    const StopArgs st{hdec + (int64_t)B * R, outp, h->ws, h->bs, tr ? m->stop : nullptr, tr ? m->scale_stop : 1.f, stop,
                      B, T, R, MR, MRP};
    hipLaunchKernelGGL(dt_stop_kernel, dim3(blocks(TB, 4)), dim3(256), 0, s, st);
    hipLaunchKernelGGL(dt_rows_out_kernel, dim3(blocks(TB * MR)), dim3(256), 0, s, outp, (int64_t)MRP, out, B, T, MR);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status tts_dectrain_backward(tts_dectrain* h, const uint8_t* mask, int B, int L, int T, const tts_dectrain_masks* m,
                                 const float* reserve, const float* grad_out, const float* grad_stop, float* grad_inputs,
                                 float* grad_memories, const tts_dectrain_grads* gw, void* stream) {
    TTS_TRY(check_shape(h, B, L, T, "dectrain_backward"));
    TTS_CHECK(reserve && m && gw, TTS_ERR_INVALID, "dectrain_backward: null reserve, masks or gradient table");
    TTS_CHECK(aligned16(reserve), TTS_ERR_INVALID, "dectrain_backward: the reserve must be 16-byte aligned");
    TTS_CHECK(m->att_h && m->att_c && m->dec_h && m->dec_c && m->stop, TTS_ERR_INVALID,
              "dectrain_backward: the dropout masks of the forward are needed");
    TTS_CHECK(grad_out || grad_stop, TTS_ERR_INVALID, "dectrain_backward: neither grad_out nor grad_stop");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int E = h->E, PN = h->PN, R = h->R, A = h->A, MR = h->MR, MRP = h->MRP, G = 4 * R, Lp = pad16(L);
    const int64_t TB = (int64_t)T * B;
    const Reserve lay = reserve_layout(h, B, L, T);
    const float* base = reserve;
    const float *hatt = base + lay.hatt, *hdec = base + lay.hdec, *ctx = base + lay.ctx, *alpha = base + lay.alpha;
    const float *q = base + lay.q, *h1 = base + lay.h1, *h2 = base + lay.h2, *fr = base + lay.fr, *outp = base + lay.outp;
    const float *P = base + lay.P, *inz = base + lay.inz;
    const bool pd = h->prenet_dropout;
    const int nsplit = (int)((TB + DT_KC - 1) / DT_KC);

    // the widest partial: a weight gradient [4R][max(R, E, PN)] per chunk, or grad_inputs [B][Lp][E]
    const int64_t widest = std::max<int64_t>({(int64_t)R, E, PN, A + 16, MRP, R + MR + 1});
    const int tsplit = (T + DT_KC - 1) / DT_KC;
    // the largest set of partials any product below writes: rows of A^T (4R, att, prenet or MRP) x the widest B
    // operand per chunk of T * B rows, grad inputs_w's [att][enc] per chunk of B * L rows, grad_inputs per sentence
    const int64_t lsplit = ((int64_t)B * L + DT_KC - 1) / DT_KC;
    const int64_t tallest = std::max<int64_t>({(int64_t)G, MRP, A, PN});
    TTS_TRY(h->partial.reserve((size_t)std::max<int64_t>(
        {(int64_t)nsplit * tallest * widest, lsplit * A * E, (int64_t)tsplit * B * Lp * E})));

    const StopArgs st{hdec + (int64_t)B * R, outp, h->ws, h->bs, m->stop, m->scale_stop, nullptr, B, T, R, MR, MRP};
    if (grad_stop && (gw->stop_w || gw->stop_b)) {
        const int K = R + MR;
        hipLaunchKernelGGL(dt_stop_wgrad_kernel, dim3(blocks(K + 1), (unsigned)nsplit), dim3(256), 0, s, st, grad_stop,
                           h->partial.p);
        TTS_HIP(hipGetLastError());
        if (gw->stop_w) {
            const FoldArgs f{h->partial.p, nsplit, 1, K + 1, 1, K, 1, gw->stop_w, K, 0, 0, nullptr, nullptr};
            hipLaunchKernelGGL(dt_fold_kernel, dim3(blocks(K)), dim3(256), 0, s, f);
        }
        if (gw->stop_b) {
            const FoldArgs f{h->partial.p + K, nsplit, 1, K + 1, 1, 1, 1, gw->stop_b, 1, 0, 0, nullptr, nullptr};
            hipLaunchKernelGGL(dt_fold_kernel, dim3(1), dim3(256), 0, s, f);
        }
        TTS_HIP(hipGetLastError());
    }
    // only the stopnet's own gradients asked for: no walk back through time
    bool walk = grad_inputs || grad_memories;
    for (const float* p : {gw->prenet_w1, gw->prenet_w2, gw->att_w_ih, gw->att_w_hh, gw->att_b_ih, gw->att_b_hh,
                           gw->query_w, gw->inputs_w, gw->v_w, gw->v_b, gw->dec_w_ih, gw->dec_w_hh, gw->dec_b_ih,
                           gw->dec_b_hh, gw->proj_w, gw->proj_b, gw->att_init, gw->go_init, gw->dec_init})
        walk = walk || p;
    if (!walk) return TTS_OK;
    const float* dstop_in = (!h->separate && grad_stop) ? grad_stop : nullptr;  // the stopnet's input gradient joins

    // workspace of the backward
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += (n + 3) / 4 * 4;
        return at;
    };
    const int64_t o_dpa = take(TB * G), o_dpd = take(TB * G), o_dhc = take(TB * (R + E)), o_dout = take(TB * MRP),
                  o_dx = take((int64_t)B * (R + E)), o_dcc = take((int64_t)B * E), o_dal = take((int64_t)B * Lp),
                  o_dq = take(TB * A), o_dvp = take(TB * (A + 16)), o_dP = take((int64_t)B * L * A),
                  o_dca = take((int64_t)B * R), o_dcd = take((int64_t)B * R), o_d2 = take(TB * PN), o_d1 = take(TB * PN),
                  o_dfr = take(TB * MRP), o_di = take((int64_t)B * R);
    TTS_TRY(h->bws.reserve((size_t)o));
    float* w = h->bws.p;
    float *dpa = w + o_dpa, *dpd = w + o_dpd, *dhc = w + o_dhc, *dout = w + o_dout, *dx = w + o_dx, *dcc = w + o_dcc;
    float *dal = w + o_dal, *dq = w + o_dq, *dvp = w + o_dvp, *dP = w + o_dP, *dca = w + o_dca, *dcd = w + o_dcd;
    float *d2 = w + o_d2, *d1 = w + o_d1, *dfr = w + o_dfr, *dinit = w + o_di;

    hipLaunchKernelGGL(dt_dout_kernel, dim3(blocks(TB * MRP)), dim3(256), 0, s, st, grad_out, dstop_in, dout);
    TTS_TRY(nt_gemm(dout, MRP, MRP, nullptr, 0, 0, h->wprojt, MRP, nullptr, dhc, R + E, TB, R + E, s));
    if (dstop_in) hipLaunchKernelGGL(dt_dh_stop_kernel, dim3(blocks(TB * R)), dim3(256), 0, s, st, dstop_in, dhc, (int64_t)(R + E));
    hipLaunchKernelGGL(dt_fill_kernel, dim3(blocks((int64_t)B * L * A)), dim3(256), 0, s, dP, (int64_t)B * L * A, 0.f);
    TTS_HIP(hipGetLastError());

    const size_t lds = (size_t)(4 * Lp + E + 2 * DT_AT) * sizeof(float);
    for (int t = T - 1; t >= 0; --t) {
        const int64_t row = (int64_t)t * B;
        const bool last = t == T - 1;
        StepArgs a{};  // 1: decoder LSTM back
        a.W = h->wtd_h, a.ldw = G, a.N = R, a.B = B, a.H = R;
        a.x[0] = dpd + (row + B) * G, a.ldx[0] = G, a.k[0] = G, a.act = last ? 0 : 1;
        a.add = dhc + row * (R + E), a.ldadd = R + E;
        a.cst = dcd, a.first = last;
        a.mh = m->dec_h + row * R, a.mc = m->dec_c + row * R, a.scale = m->scale_rnn;
        a.rg = const_cast<float*>(base + lay.gdec + row * R * 4), a.rc = const_cast<float*>(base + lay.cdec + row * R);
        a.cprev = t > 0 ? base + lay.cdec + (row - B) * R : nullptr, a.mcprev = t > 0 ? m->dec_c + (row - B) * R : nullptr;
        a.dpre = dpd + row * G;
        TTS_TRY(step_launch<EPI_LSTM_BWD>(a, s));

        StepArgs x{};  // 2: [dh_att | dctx] from the decoder LSTM's input
        x.W = h->wtd_x, x.ldw = G, x.N = R + E, x.B = B;
        x.x[0] = dpd + row * G, x.ldx[0] = G, x.k[0] = G, x.act = 1;
        x.C = dx, x.ldc = R + E;
        TTS_TRY(step_launch<EPI_PLAIN>(x, s));

        AttnArgs at{};  // 3
        at.q = q + row * A, at.P = P, at.inz = inz, at.v = h->v, at.bv = h->bv, at.mask = mask;
        at.aprev = t > 0 ? alpha + (row - B) * Lp : nullptr, at.alpha = const_cast<float*>(alpha + row * Lp);
        at.L = L, at.Lp = Lp, at.A = A, at.E = E, at.T = T, at.t = t, at.norm = h->norm, at.fwd = h->fwd_attn;
        at.dx = dx + R, at.lddx = R + E, at.dcc = last ? nullptr : dcc;
        at.dctx = dhc + row * (R + E) + R, at.ldc = R + E;
        at.dal = dal, at.last = last;
        at.dq = dq + row * A, at.dvp = dvp + row * (A + 16), at.dP = dP;
        hipLaunchKernelGGL(dt_attn_bwd_kernel, dim3((unsigned)B), dim3(DT_AT), lds, s, at);

        StepArgs b{};  // 4: attention LSTM back
        b.W = h->wta_h, b.ldw = A + G, b.N = R, b.B = B, b.H = R;
        b.x[0] = dq + row * A, b.ldx[0] = A, b.k[0] = A;
        b.x[1] = dpa + (row + B) * G, b.ldx[1] = G, b.k[1] = G;
        b.act = last ? 1 : 3;
        b.add = dx, b.ldadd = R + E;
        b.cst = dca, b.first = last;
        b.mh = m->att_h + row * R, b.mc = m->att_c + row * R, b.scale = m->scale_rnn;
        b.rg = const_cast<float*>(base + lay.gatt + row * R * 4), b.rc = const_cast<float*>(base + lay.catt + row * R);
        b.cprev = t > 0 ? base + lay.catt + (row - B) * R : nullptr, b.mcprev = t > 0 ? m->att_c + (row - B) * R : nullptr;
        b.dpre = dpa + row * G;
        TTS_TRY(step_launch<EPI_LSTM_BWD>(b, s));

        if (t > 0) {  // 5: the context's gradient carried into step t - 1
            StepArgs c{};
            c.W = h->wta_c, c.ldw = G, c.N = E, c.B = B;
            c.x[0] = dpa + row * G, c.ldx[0] = G, c.k[0] = G, c.act = 1;
            c.C = dcc, c.ldc = E;
            TTS_TRY(step_launch<EPI_PLAIN>(c, s));
        }
    }
    TTS_HIP(hipGetLastError());

    // ---- everything that does not feed the recurrence
    // the three one-row embeddings: dh of the initial states, summed over the batch
    if (gw->att_init) {
        StepArgs c{};
        c.W = h->wta_h + A, c.ldw = A + G, c.N = R, c.B = B;
        c.x[0] = dpa, c.ldx[0] = G, c.k[0] = G, c.act = 1;
        c.C = dinit, c.ldc = R;
        TTS_TRY(step_launch<EPI_PLAIN>(c, s));
        TTS_TRY(col_sum(h, dinit, R, B, R, gw->att_init, R, s));
    }
    if (gw->dec_init) {
        StepArgs c{};
        c.W = h->wtd_h, c.ldw = G, c.N = R, c.B = B;
        c.x[0] = dpd, c.ldx[0] = G, c.k[0] = G, c.act = 1;
        c.C = dinit, c.ldc = R;
        TTS_TRY(step_launch<EPI_PLAIN>(c, s));
        TTS_TRY(col_sum(h, dinit, R, B, R, gw->dec_init, R, s));
    }
    // LSTM weights: dpre^T [operands of the step]
    TTS_TRY(tn_product(h, dpa, G, G, h2, PN, PN, TB, gw->att_w_ih, PN + E, 0, G, PN, s));
    if (gw->att_w_ih) {
        if (T > 1)
            TTS_TRY(tn_product(h, dpa + (int64_t)B * G, G, G, ctx, E, E, TB - B, gw->att_w_ih, PN + E, PN, G, E, s));
        else
            hipLaunchKernelGGL(dt_copy2d_kernel, dim3(blocks((int64_t)G * E)), dim3(256), 0, s,
                               CopyArgs{dpa, G, 0, G, E, 0, gw->att_w_ih, PN + E, PN, 0, 0});  // (zeros: ctx_{-1} = 0)
    }
    TTS_TRY(tn_product(h, dpa, G, G, hatt, R, R, TB, gw->att_w_hh, R, 0, G, R, s));
    TTS_TRY(col_sum(h, dpa, G, TB, G, gw->att_b_ih, G, s));
    TTS_TRY(col_sum(h, dpa, G, TB, G, gw->att_b_hh, G, s));
    TTS_TRY(tn_product(h, dpd, G, G, hatt + (int64_t)B * R, R, R, TB, gw->dec_w_ih, R + E, 0, G, R, s));
    TTS_TRY(tn_product(h, dpd, G, G, ctx, E, E, TB, gw->dec_w_ih, R + E, R, G, E, s));
    TTS_TRY(tn_product(h, dpd, G, G, hdec, R, R, TB, gw->dec_w_hh, R, 0, G, R, s));
    TTS_TRY(col_sum(h, dpd, G, TB, G, gw->dec_b_ih, G, s));
    TTS_TRY(col_sum(h, dpd, G, TB, G, gw->dec_b_hh, G, s));
    // attention
    TTS_TRY(tn_product(h, dq, A, A, hatt + (int64_t)B * R, R, R, TB, gw->query_w, R, 0, A, R, s));
    TTS_TRY(tn_product(h, dP, A, A, inz, E, E, (int64_t)B * L, gw->inputs_w, E, 0, A, E, s));
    TTS_TRY(col_sum(h, dvp, A + 16, TB, A, gw->v_w, A, s));
    TTS_TRY(col_sum(h, dvp + A, A + 16, TB, 1, gw->v_b, 1, s));
    // projection
    TTS_TRY(tn_product(h, dout, MRP, MRP, hdec + (int64_t)B * R, R, R, TB, gw->proj_w, R + E, 0, MR, R, s));
    TTS_TRY(tn_product(h, dout, MRP, MRP, ctx, E, E, TB, gw->proj_w, R + E, R, MR, E, s));
    TTS_TRY(col_sum(h, dout, MRP, TB, MRP, gw->proj_b, MR, s));
    // prenet
    if (gw->prenet_w1 || gw->prenet_w2 || gw->go_init || grad_memories) {
        TTS_TRY(nt_gemm(dpa, G, G, nullptr, 0, 0, h->wapt, G, nullptr, d2, PN, TB, PN, s));
        hipLaunchKernelGGL(dt_relu_drop_bwd_kernel, dim3(blocks(TB * PN)), dim3(256), 0, s, d2, h2,
                           pd ? m->scale_prenet : 1.f, TB * PN);
        TTS_TRY(tn_product(h, d2, PN, PN, h1, PN, PN, TB, gw->prenet_w2, PN, 0, PN, PN, s));
        TTS_TRY(nt_gemm(d2, PN, PN, nullptr, 0, 0, h->w2t, PN, nullptr, d1, PN, TB, PN, s));
        hipLaunchKernelGGL(dt_relu_drop_bwd_kernel, dim3(blocks(TB * PN)), dim3(256), 0, s, d1, h1,
                           pd ? m->scale_prenet : 1.f, TB * PN);
        TTS_TRY(tn_product(h, d1, PN, PN, fr, MRP, MRP, TB, gw->prenet_w1, MR, 0, PN, MR, s));
        if (gw->go_init || grad_memories) {
            TTS_TRY(nt_gemm(d1, PN, PN, nullptr, 0, 0, h->w1t, PN, nullptr, dfr, MRP, TB, MRP, s));
            TTS_TRY(col_sum(h, dfr, MRP, B, MRP, gw->go_init, MR, s));
            if (grad_memories)
                hipLaunchKernelGGL(dt_gmem_kernel, dim3(blocks(TB * MR)), dim3(256), 0, s, dfr, grad_memories, B, T, MR, MRP);
        }
    }
    // grad_inputs = dP Wp + sum_t alpha_t^T dctx_t; masked rows +0.0
    if (grad_inputs) {
        TTS_TRY(nt_gemm(dP, A, A, nullptr, 0, 0, h->wpt, A, nullptr, grad_inputs, E, (int64_t)B * L, E, s));
        const TnArgs t{alpha, (int64_t)B * Lp, Lp, dhc + R, (int64_t)B * (R + E), R + E, h->partial.p, Lp, E, T, tsplit};
        hipLaunchKernelGGL(dt_tn_partial_kernel,
                           dim3((unsigned)((E + 63) / 64), (unsigned)((Lp + 63) / 64), (unsigned)(B * tsplit)), dim3(64), 0,
                           s, t);
        const FoldArgs f{h->partial.p, tsplit, Lp, E, L, E, B, grad_inputs, E, (int64_t)L * E, 0, grad_inputs, mask};
        hipLaunchKernelGGL(dt_fold_kernel, dim3(blocks((int64_t)B * L * E)), dim3(256), 0, s, f);
    }
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

}  // extern "C"
