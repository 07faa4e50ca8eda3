// The reference's evaluation losses on tensors in HBM:
//   L1LossMasked / MSELossMasked (layers/losses.py:7-62): input * mask, target * mask, l1_loss / mse_loss
//     with reduction="sum", divided by mask.sum(); nn.L1Loss / nn.MSELoss (train.py:464) when no lengths
//     are given; nn.BCEWithLogitsLoss on the stop logits (train.py:465).
// A streaming reduction, HBM-bound: every valid element of both operands is read once (8 bytes per
// term, ~3 fp64 operations), nothing is written but one fp64 partial per workgroup.
//
// Work: sentence b's valid region is one flat run of n_b = min(lengths[b], T) * D floats.  It is cut
// into chunks of LOSS_CHUNK elements BY ELEMENT INDEX, one workgroup per chunk: the grid is the number
// of chunks of the whole batch (a long sentence spreads over many compute units, a sentence without
// valid rows gets no workgroup).  A workgroup finds its sentence by bisection over the first-chunk
// prefix table.  Rows at and beyond a sentence's length are never read.
//
// Order: thread t of a chunk takes the quads t, t + 256, ... of the chunk, component c of every quad
// into accumulator c, then (a0 + a1) + (a2 + a3), an xor butterfly over the wave, the waves in index
// order: one fp64 partial per chunk.  The second launch folds each sentence's partials (lane l takes
// partials l, l + 64, ... in order, then the butterfly), then the sentences in the same way.  Which term
// meets which is a function of the element index alone, so the three results are bitwise the same run to
// run and whatever the operands' pitches or base addresses are.  That is also why the 16-byte loads sit
// at element indices that are multiples of four of the sentence and not at 16-byte aligned addresses: an
// aligned-middle split would move terms between threads with the base address (at D = 1025 a sentence's
// base is 16-byte aligned only by chance).  The loads are declared 4-byte aligned; gfx950 serves a
// dword-aligned global_load_dwordx4, and an aligned base costs nothing extra.  Only a chunk's last,
// partial quad is loaded by scalars.  No floating-point atomics, no in-launch hand-off between workgroups.
//
// The criteria's gradient for loss.backward() (train.py:157) is the third kernel, further down.
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_util.h"

namespace tts {
namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / WAVE;
constexpr int LOSS_QUADS = 8;                               // 16-byte loads per thread and operand
constexpr int LOSS_CHUNK = LOSS_THREADS * 4 * LOSS_QUADS;   // elements per workgroup (2 x 32 KiB read)
constexpr int FOLD_THREADS = 1024;                          // the fold: one workgroup, a wave per sentence in turn
constexpr int KIND_BCE = TTS_LOSS_BCE;                      // the forward has its own entry point for it

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

struct LossArgs {
    const float* x;        // input / logits
    const float* y;        // target
    int64_t x_pitch, y_pitch;
    const int64_t* n;      // [B] valid elements per sentence
    const int* first;      // [B + 1] first chunk of each sentence, [B] = chunks in all
    int B;
    double* partial;       // [chunks]
};

// the fp64 term of one element pair, from the fp32 operands
template <int KIND>
__device__ __forceinline__ double loss_term(float xf, float yf) {
    const double x = (double)xf, y = (double)yf;
    if (KIND == TTS_LOSS_L1) return fabs(x - y);
    if (KIND == TTS_LOSS_MSE) {
        const double d = x - y;
        return d * d;
    }
    // BCEWithLogitsLoss: max(x, 0) - x y + log1p(exp(-|x|)); exp's argument is <= 0, so no overflow
    return fmax(x, 0.0) - x * y + log1p(exp(-fabs(x)));
}

template <int KIND>
__global__ __launch_bounds__(LOSS_THREADS) void loss_partial_kernel(const LossArgs a) {
    __shared__ double sw[LOSS_WAVES];
    const int blk = blockIdx.x;
    int lo = 0, hi = a.B;  // first[lo] <= blk < first[hi]: the last sentence that starts at or before blk
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= blk) lo = mid;
        else hi = mid;
    }
    const int b = lo;
    const int64_t start = (int64_t)(blk - a.first[b]) * LOSS_CHUNK;
    const int64_t left = a.n[b] - start;  // >= 1: the host counted this chunk
    const int cnt = left < LOSS_CHUNK ? (int)left : LOSS_CHUNK;
    const float* x = a.x + (int64_t)b * a.x_pitch + start;
    const float* y = a.y + (int64_t)b * a.y_pitch + start;
    const int tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (cnt == LOSS_CHUNK) {  // (block-uniform) every load in flight before the first term
        float4u vx[LOSS_QUADS], vy[LOSS_QUADS];
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int e = 4 * (tid + j * LOSS_THREADS);
            vx[j] = *reinterpret_cast<const float4u*>(x + e);
            vy[j] = *reinterpret_cast<const float4u*>(y + e);
        }
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += loss_term<KIND>(vx[j][c], vy[j][c]);
    } else {
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int e = 4 * (tid + j * LOSS_THREADS);
            if (e + 4 <= cnt) {
                const float4u vx = *reinterpret_cast<const float4u*>(x + e);
                const float4u vy = *reinterpret_cast<const float4u*>(y + e);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] += loss_term<KIND>(vx[c], vy[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (e + c < cnt) acc[c] += loss_term<KIND>(x[e + c], y[e + c]);
            }
        }
    }
    const double s = wave_sum_f64((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((tid & (WAVE - 1)) == 0) sw[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = sw[0];
        for (int w = 1; w < LOSS_WAVES; ++w) t += sw[w];
        a.partial[blk] = t;
    }
}

struct FoldArgs {
    const double* partial;
    const int* first;
    int B;
    long long count;       // number of terms
    double* per_sentence;  // [B]
    double* scal;          // [2] total sum, loss
    float* loss32;
};

// v[0 .. n) by one wave: lane l adds l, l + 64, ... in index order, then the butterfly
__device__ __forceinline__ double wave_fold(const double* v, int n, int lane) {
    double s = 0.0;
    for (int i = lane; i < n; i += WAVE) s += v[i];
    return wave_sum_f64(s);
}

__global__ __launch_bounds__(FOLD_THREADS) void loss_fold_kernel(const FoldArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    for (int b = w; b < a.B; b += FOLD_THREADS / WAVE) {
        const double s = wave_fold(a.partial + a.first[b], a.first[b + 1] - a.first[b], lane);
        if (lane == 0) a.per_sentence[b] = s;
    }
    __syncthreads();  // (one workgroup: the sums above are visible to wave 0)
    if (w != 0) return;
    const double total = wave_fold(a.per_sentence, a.B, lane);
    if (lane == 0) {
        const double loss = total / (double)a.count;  // count 0: 0 / 0 = NaN, as the reference's
        a.scal[0] = total;
        a.scal[1] = loss;
        *a.loss32 = (float)loss;  // the fp64 value rounded once
    }
}

// ---------------------------------------------------------------- the gradient (train.py:157)
// d loss / d input of the five criteria, elementwise: 8 bytes read and 4 written per valid element, 4
// written per padding element, no reduction, no atomics, no hand-off.  The same cut as the forward
// (LOSS_CHUNK elements by element index within a sentence, 16-byte accesses at element indices that are
// multiples of four of the sentence, declared 4-byte aligned, a chunk's last partial quad by scalars), but
// the grid covers every chunk of [B][T * D]: padding gets its zeros.  A chunk is entirely valid (all loads
// in flight before the first value), entirely padding (stores only) or straddles n[b]; which, is
// block-uniform.  x and y are never read at or beyond n[b].
struct GradArgs {
    const float* x;        // input / logits
    const float* y;        // target
    int64_t x_pitch, y_pitch;
    const int64_t* n;      // [B] valid elements per sentence, or null: per each
    int64_t per;           // T * D
    int chunks_per;        // chunks per sentence
    long long count;       // number of terms of the forward
    const float* gout;     // device scalar, or null: 1
    float* g;              // grad_input
    int64_t g_pitch;
};

// the fp64 gradient of one element pair, rounded to fp32 once; scale = gout / count
template <int KIND>
__device__ __forceinline__ float loss_grad(float xf, float yf, double scale) {
    const double x = (double)xf, y = (double)yf;
    if (KIND == TTS_LOSS_L1) {
        const double d = x - y;
        return (float)(scale * (d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0));  // sign(0) = 0, as torch's l1_loss backward
    }
    if (KIND == TTS_LOSS_MSE) return (float)(scale * (2.0 * (x - y)));
    // BCEWithLogitsLoss: sigmoid(x) - y; exp's argument is <= 0, so no overflow
    double sg;
    if (x >= 0.0) sg = 1.0 / (1.0 + exp(-x));
    else {
        const double e = exp(x);
        sg = e / (1.0 + e);
    }
    return (float)(scale * (sg - y));
}

template <int KIND>
__global__ __launch_bounds__(LOSS_THREADS) void loss_grad_kernel(const GradArgs a) {
    const int b = blockIdx.x / a.chunks_per;
    const int64_t start = (int64_t)(blockIdx.x - b * a.chunks_per) * LOSS_CHUNK;
    const int64_t room = a.per - start;  // >= 1: elements of [T * D] from this chunk's start on
    const int cnt = room < LOSS_CHUNK ? (int)room : LOSS_CHUNK;
    int64_t nb = a.n ? a.n[b] : a.per;
    nb = nb < 0 ? 0 : nb > a.per ? a.per : nb;  // (a table out of range must not move an access out of [T * D])
    const int64_t left = nb - start;
    const int valid = left <= 0 ? 0 : left < cnt ? (int)left : cnt;
    const float* x = a.x + (int64_t)b * a.x_pitch + start;
    const float* y = a.y + (int64_t)b * a.y_pitch + start;
    float* g = a.g + (int64_t)b * a.g_pitch + start;
    const int tid = threadIdx.x;
    // count 0: the reference's 1 / mask.sum() is inf and inf * 0 NaN on every element (all are padding then)
    const float pad = a.count == 0 ? __builtin_nanf("") : 0.0f;
    const float4u pad4 = {pad, pad, pad, pad};
    if (valid == 0) {  // (block-uniform) padding only: nothing is loaded, not even grad_output
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int e = 4 * (tid + j * LOSS_THREADS);
            if (e + 4 <= cnt) *reinterpret_cast<float4u*>(g + e) = pad4;
            else
                for (int c = 0; c < 4; ++c)
                    if (e + c < cnt) g[e + c] = pad;
        }
        return;
    }
    const double scale = (a.gout ? (double)*a.gout : 1.0) / (double)a.count;
    if (valid == LOSS_CHUNK) {  // (block-uniform) every load in flight before the first value
        float4u vx[LOSS_QUADS], vy[LOSS_QUADS];
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int e = 4 * (tid + j * LOSS_THREADS);
            vx[j] = *reinterpret_cast<const float4u*>(x + e);
            vy[j] = *reinterpret_cast<const float4u*>(y + e);
        }
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j) {
            float4u v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = loss_grad<KIND>(vx[j][c], vy[j][c], scale);
            *reinterpret_cast<float4u*>(g + 4 * (tid + j * LOSS_THREADS)) = v;
        }
        return;
    }
    for (int j = 0; j < LOSS_QUADS; ++j) {  // the chunk that holds n[b], or the sentence's last one
        const int e = 4 * (tid + j * LOSS_THREADS);
        if (e + 4 <= valid) {
            const float4u vx = *reinterpret_cast<const float4u*>(x + e);
            const float4u vy = *reinterpret_cast<const float4u*>(y + e);
            float4u v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = loss_grad<KIND>(vx[c], vy[c], scale);
            *reinterpret_cast<float4u*>(g + e) = v;
        } else if (e >= valid && e + 4 <= cnt) {
            *reinterpret_cast<float4u*>(g + e) = pad4;
        } else {
            for (int c = 0; c < 4; ++c) {
                if (e + c < valid) g[e + c] = loss_grad<KIND>(x[e + c], y[e + c], scale);
                else if (e + c < cnt) g[e + c] = pad;
            }
        }
    }
}

}  // namespace
}  // namespace tts

// The partials workspace (grown on demand, by the chunks of the call and its batch) and the host copy
// of the per-sentence table for the upload.  Every call waits for its stream, so the block is idle
// whenever a call begins.
struct tts_loss {
    tts::DeviceBuf<char> ws;
    std::vector<char> host;
};

namespace tts {
namespace {

// n[b] valid elements per sentence -> partials -> per-sentence sums, total and loss; waits for s
tts_status loss_run(tts_loss* h, int kind, const float* x, int64_t x_pitch, const float* y, int64_t y_pitch,
                    const std::vector<int64_t>& n, double* per_sentence, float* loss_dev, double* sum_out,
                    int64_t* count_out, double* loss_out, hipStream_t s) {
    const int B = (int)n.size();
    std::vector<int> first(B + 1, 0);
    int64_t chunks = 0, count = 0;
    for (int b = 0; b < B; ++b) {
        chunks += (n[b] + LOSS_CHUNK - 1) / LOSS_CHUNK;
        count += n[b];
        TTS_CHECK(chunks <= INT32_MAX, TTS_ERR_INVALID, "loss: more than 2^31 - 1 chunks of work");
        first[b + 1] = (int)chunks;
    }
    // [chunks] partials, [2] scalars, [B] n, [B + 1] first
    const size_t off_scal = (size_t)chunks * sizeof(double), off_n = off_scal + 2 * sizeof(double);
    const size_t off_first = off_n + (size_t)B * sizeof(int64_t), bytes = off_first + (size_t)(B + 1) * sizeof(int);
    TTS_TRY(h->ws.reserve(bytes));
    h->host.resize(bytes - off_n);
    std::copy(n.begin(), n.end(), reinterpret_cast<int64_t*>(h->host.data()));
    std::copy(first.begin(), first.end(), reinterpret_cast<int*>(h->host.data() + (off_first - off_n)));
    TTS_HIP(hipMemcpyAsync(h->ws.p + off_n, h->host.data(), bytes - off_n, hipMemcpyHostToDevice, s));
    double* partial = reinterpret_cast<double*>(h->ws.p);
    double* scal = reinterpret_cast<double*>(h->ws.p + off_scal);
    const int64_t* n_dev = reinterpret_cast<const int64_t*>(h->ws.p + off_n);
    const int* first_dev = reinterpret_cast<const int*>(h->ws.p + off_first);
    if (chunks > 0) {  // (0: no sentence has a valid row)
        LossArgs a{x, y, x_pitch, y_pitch, n_dev, first_dev, B, partial};
        const dim3 grid((unsigned)chunks), block(LOSS_THREADS);
        if (kind == TTS_LOSS_L1) hipLaunchKernelGGL(loss_partial_kernel<TTS_LOSS_L1>, grid, block, 0, s, a);
        else if (kind == TTS_LOSS_MSE) hipLaunchKernelGGL(loss_partial_kernel<TTS_LOSS_MSE>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(loss_partial_kernel<KIND_BCE>, grid, block, 0, s, a);
        TTS_HIP(hipGetLastError());
    }
    FoldArgs f{partial, first_dev, B, (long long)count, per_sentence, scal, loss_dev};
    hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, s, f);
    TTS_HIP(hipGetLastError());
    double back[2];
    TTS_HIP(hipMemcpyAsync(back, scal, sizeof(back), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipStreamSynchronize(s));
    *sum_out = back[0];
    *count_out = count;
    *loss_out = back[1];
    return TTS_OK;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_loss_create(tts_loss** out) {
    TTS_CHECK(out, TTS_ERR_INVALID, "loss_create: null argument");
    *out = new tts_loss();
    return TTS_OK;
}

void tts_loss_destroy(tts_loss* h) {
    if (!h) return;
    if (h->ws.p) (void)hipFree(h->ws.p);
    delete h;
}

tts_status tts_loss_masked(tts_loss* h, int kind, const float* input, int64_t input_pitch, const float* target,
                           int64_t target_pitch, const int32_t* lengths, int B, int T, int D, double* per_sentence,
                           float* loss_dev, double* sum_out, int64_t* count_out, double* loss_out, void* stream) {
    TTS_CHECK(h && input && target && per_sentence && loss_dev && sum_out && count_out && loss_out, TTS_ERR_INVALID,
              "loss_masked: null argument");
    TTS_CHECK(kind == TTS_LOSS_L1 || kind == TTS_LOSS_MSE, TTS_ERR_INVALID, "loss_masked: kind must be L1 or MSE");
    TTS_CHECK(B >= 1 && T >= 1 && D >= 1, TTS_ERR_INVALID, "loss_masked: B, T and D must be positive");
    TTS_CHECK(input_pitch >= (int64_t)T * D && target_pitch >= (int64_t)T * D, TTS_ERR_INVALID,
              "loss_masked: a batch pitch is below T * D");
    std::vector<int64_t> n(B, (int64_t)T * D);
    for (int b = 0; lengths && b < B; ++b) {
        TTS_CHECK(lengths[b] >= 0, TTS_ERR_INVALID,
                  "loss_masked: sentence " + std::to_string(b) + " has a negative length");
        n[b] = (int64_t)std::min(lengths[b], T) * D;
    }
    return loss_run(h, kind, input, input_pitch, target, target_pitch, n, per_sentence, loss_dev, sum_out, count_out,
                    loss_out, static_cast<hipStream_t>(stream));
}

tts_status tts_loss_bce_logits(tts_loss* h, const float* logits, const float* targets, int64_t n, double* sum_dev,
                               float* loss_dev, double* sum_out, double* loss_out, void* stream) {
    TTS_CHECK(h && logits && targets && sum_dev && loss_dev && sum_out && loss_out, TTS_ERR_INVALID,
              "loss_bce_logits: null argument");
    TTS_CHECK(n >= 1, TTS_ERR_INVALID, "loss_bce_logits: n must be positive");
    int64_t count;
    return loss_run(h, KIND_BCE, logits, 0, targets, 0, std::vector<int64_t>(1, n), sum_dev, loss_dev, sum_out, &count,
                    loss_out, static_cast<hipStream_t>(stream));
}

tts_status tts_loss_backward(int kind, const float* input, int64_t input_pitch, const float* target,
                             int64_t target_pitch, const int64_t* n_valid, int B, int64_t per_sentence, int64_t count,
                             const float* grad_output, float* grad_input, int64_t grad_pitch, void* stream) {
    TTS_CHECK(input && target && grad_input, TTS_ERR_INVALID, "loss_backward: null argument");
    TTS_CHECK(kind == TTS_LOSS_L1 || kind == TTS_LOSS_MSE || kind == TTS_LOSS_BCE, TTS_ERR_INVALID,
              "loss_backward: kind must be L1, MSE or BCE");
    TTS_CHECK(B >= 1 && per_sentence >= 1, TTS_ERR_INVALID, "loss_backward: B and per_sentence must be positive");
    TTS_CHECK(input_pitch >= per_sentence && target_pitch >= per_sentence && grad_pitch >= per_sentence,
              TTS_ERR_INVALID, "loss_backward: a batch pitch is below per_sentence");
    TTS_CHECK(count >= 0, TTS_ERR_INVALID, "loss_backward: count is negative");
    const int64_t chunks_per = (per_sentence + LOSS_CHUNK - 1) / LOSS_CHUNK;
    TTS_CHECK(chunks_per * B <= INT32_MAX, TTS_ERR_INVALID, "loss_backward: more than 2^31 - 1 chunks of work");
    GradArgs a{input, target, input_pitch, target_pitch, n_valid, per_sentence, (int)chunks_per, (long long)count,
               grad_output, grad_input, grad_pitch};
    const dim3 grid((unsigned)(chunks_per * B)), block(LOSS_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (kind == TTS_LOSS_L1) hipLaunchKernelGGL(loss_grad_kernel<TTS_LOSS_L1>, grid, block, 0, s, a);
    else if (kind == TTS_LOSS_MSE) hipLaunchKernelGGL(loss_grad_kernel<TTS_LOSS_MSE>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(loss_grad_kernel<TTS_LOSS_BCE>, grid, block, 0, s, a);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

}  // extern "C"
