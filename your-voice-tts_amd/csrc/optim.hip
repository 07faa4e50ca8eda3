// The tail of the reference's training iteration on parameters in HBM (train.py:157-167):
//   weight_decay(optimizer, wd)      p <- p + (-wd * lr) * p                 (utils/generic_utils.py:174-182)
//   check_update(model, grad_clip)   clip_grad_norm_, in place               (utils/generic_utils.py:155-162)
//   optimizer.step()                 torch.optim.Adam, weight_decay = 0      (train.py:454-457)
// A streaming job, HBM-bound: the norm pass reads g once (4 bytes per element), the update pass reads
// p, g, m, v once and writes p, m, v once (28 bytes per element, 32 when the clip scales g in place).
//
// Work: every tensor is cut into chunks of TTS_OPTIM_CHUNK elements by element index.  The chunk -> (tensor,
// chunk of the tensor) map is built on the host when the sizes are set and lives on the device; the table of
// pointers and per-tensor fp32 scalars goes up on the stream with every call (autograd gives .grad a new
// address after zero_grad(set_to_none=True)).  One launch covers every tensor: at most OPT_MAX_GRID
// workgroups, each striding over the chunks.
//
// Order, norm: thread t of a chunk takes the quads t, t + 256, ... of the chunk, component c of every quad
// into fp64 accumulator c (g * g formed in fp64 from the fp32 operand), then (a0 + a1) + (a2 + a3), an xor
// butterfly over the wave, the waves in index order: one fp64 partial per chunk.  The fold launch (one
// workgroup) gives thread t the partials t, t + 1024, ... in order, then the butterfly, then the waves in
// order.  Which term meets which is a function of (tensor, element index) alone: bitwise the same run to
// run and for any base addresses.  No floating-point atomics, no hand-off inside a launch.
//
// Paths: a chunk whose base addresses (of the arrays the launch touches) are all 16-byte aligned moves
// whole quads with 16-byte loads and stores; any other chunk (a view at an odd element offset) and a
// chunk's last, partial quad move single floats.  The element -> thread map and the arithmetic are the
// same on both, so the bits are.
//
// Arithmetic per element, fp32, no contraction (-ffp-contract=off), IEEE divide and square root, in this
// order (w1 = 1 - beta1, w2 = 1 - beta2, each scalar computed in double on the host and rounded once):
//   1. p = p + dlr * p                          dlr = float(-wd * lr); not done at all when wd == 0
//   2. g = g * coef, stored                     only when coef != 1.0f (clip_grad_norm_ multiplies by a
//                                               coefficient clamped to 1: the product by 1.0f is the operand)
//   3. m = m + w1 * (g - m)                     exp_avg.lerp_(grad, w1), ATen's form for a weight < 0.5;
//      (m = g - (g - m) * (1 - w1) for w1 >= 0.5)
//      v = v * beta2;  v = v + (w2 * g) * g     exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=w2)
//      d = sqrt(v) / sqrt(bc2) + eps            (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//      p = p + (nstep * m) / d                  param.addcdiv_(exp_avg, denom, value=-(lr / bc1))
// A tensor whose g is null is left alone by 2 and 3 and does not count in the norm (torch skips a parameter
// without a gradient); 1 applies to it, as the reference's loop over param_groups has no such test.
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_util.h"

namespace tts {
namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_WAVES = OPT_THREADS / WAVE;
constexpr int OPT_QUADS = TTS_OPTIM_CHUNK / (OPT_THREADS * 4);  // 16-byte moves per thread, array and chunk
constexpr int OPT_MAX_GRID = 2048;                              // 8 workgroups of 256 on each of 256 CUs
constexpr int OPT_FOLD_THREADS = 1024;
constexpr int OPT_RING = 4;  // pinned copies of the table in flight before a call waits for the oldest
constexpr int F_DECAY = 1, F_CLIP = 2, F_ADAM = 4;
static_assert(OPT_QUADS * OPT_THREADS * 4 == TTS_OPTIM_CHUNK, "a chunk is a whole number of quads per thread");

typedef float float4a __attribute__((ext_vector_type(4)));  // 16-byte aligned

// The table's pointers come out of memory, so the compiler cannot tell that they are global: said here, the
// moves are global_load / global_store and not their flat forms.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) float4a gfloat4;
__device__ __forceinline__ float4a ld4(const float* q) { return *(const gfloat4*)q; }
__device__ __forceinline__ void st4(float* q, float4a x) { *(gfloat4*)q = x; }
__device__ __forceinline__ float ld1(const float* q) { return *(const gfloat*)q; }
__device__ __forceinline__ void st1(float* q, float x) { *(gfloat*)q = x; }

// One tensor of a call, as the kernels read it.
struct Row {
    float *p, *g, *m, *v;
    int64_t numel;
    float dlr, w1, omw1, beta2, w2, sqrt_bc2, nstep, eps;
};

struct NormArgs {
    const Row* rows;
    const int* c_tensor;  // [chunks] tensor of the chunk
    const int* c_index;   // [chunks] its index within the tensor
    int chunks;
    double* partial;  // [chunks]
};

__global__ __launch_bounds__(OPT_THREADS) void optim_sumsq_kernel(const NormArgs a) {
    __shared__ double sw[OPT_WAVES];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < a.chunks; c += gridDim.x) {  // (block-uniform)
        const Row& r = a.rows[a.c_tensor[c]];
        const float* g0 = r.g;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (g0) {
            const int64_t start = (int64_t)a.c_index[c] * TTS_OPTIM_CHUNK;
            const int64_t left = r.numel - start;  // >= 1: the host counted this chunk
            const int cnt = left < TTS_OPTIM_CHUNK ? (int)left : TTS_OPTIM_CHUNK;
            const float* g = g0 + start;
            const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
#pragma unroll
            for (int j = 0; j < OPT_QUADS; ++j) {
                const int e = 4 * (tid + j * OPT_THREADS);
                if (vec && e + 4 <= cnt) {
                    const float4a x = ld4(g + e);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] += (double)x[k] * (double)x[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k < cnt) {
                            const double x = (double)ld1(g + e + k);
                            acc[k] += x * x;
                        }
                }
            }
        }
        const double s = wave_sum_f64((acc[0] + acc[1]) + (acc[2] + acc[3]));
        if ((tid & (WAVE - 1)) == 0) sw[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            double t = sw[0];
            for (int w = 1; w < OPT_WAVES; ++w) t += sw[w];
            a.partial[c] = t;  // 0 for a tensor without a gradient
        }
        __syncthreads();  // sw is free for the next chunk
    }
}

struct FoldArgs {
    const double* partial;
    int chunks;
    double max_norm;
    double* norm64;  // [2] sum of squares, norm
    float* norm32;   // [2] norm rounded once, clip coefficient
};

__global__ __launch_bounds__(OPT_FOLD_THREADS) void optim_fold_kernel(const FoldArgs a) {
    __shared__ double sw[OPT_FOLD_THREADS / WAVE];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < a.chunks; i += OPT_FOLD_THREADS) s += a.partial[i];
    s = wave_sum_f64(s);
    if ((tid & (WAVE - 1)) == 0) sw[tid >> 6] = s;
    __syncthreads();
    if (tid != 0) return;
    double sumsq = sw[0];
    for (int w = 1; w < OPT_FOLD_THREADS / WAVE; ++w) sumsq += sw[w];
    const double norm = sqrt(sumsq);
    // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamped to at most 1.  norm = inf gives 0 (and
    // inf * 0 = NaN in the update), a NaN norm a NaN coefficient: the clamp keeps a NaN, as torch's does.
    const double q = a.max_norm / (norm + 1e-6);
    a.norm64[0] = sumsq;
    a.norm64[1] = norm;
    a.norm32[0] = (float)norm;
    a.norm32[1] = q >= 1.0 ? 1.0f : (float)q;
}

struct UpdateArgs {
    const Row* rows;
    const int* c_tensor;
    const int* c_index;
    int chunks;
    int flags;
    const float* coef;  // the fold's clip coefficient (F_CLIP)
};

struct Scalars {
    float dlr, coef, w1, omw1, beta2, w2, sqrt_bc2, nstep, eps;
    bool decay, clip, adam;
};

__device__ __forceinline__ void update_element(const Scalars& s, float& p, float& g, float& m, float& v) {
    if (s.decay) p = p + s.dlr * p;
    if (s.clip) g = g * s.coef;
    if (s.adam) {
        const float d = g - m;
        m = s.w1 < 0.5f ? m + s.w1 * d : g - d * s.omw1;
        v = v * s.beta2;
        v = v + (s.w2 * g) * g;
        const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
        p = p + (s.nstep * m) / denom;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const UpdateArgs a) {
    const int tid = threadIdx.x;
    const float coef = (a.flags & F_CLIP) ? *a.coef : 1.0f;
    for (int c = blockIdx.x; c < a.chunks; c += gridDim.x) {  // (block-uniform, as every branch on s below)
        const Row& r = a.rows[a.c_tensor[c]];
        const bool has_g = r.g != nullptr;
        Scalars s;
        s.decay = (a.flags & F_DECAY) != 0;
        s.clip = (a.flags & F_CLIP) && has_g && coef != 1.0f;
        s.adam = (a.flags & F_ADAM) && has_g;
        if (!s.decay && !s.clip && !s.adam) continue;
        s.dlr = r.dlr, s.coef = coef, s.w1 = r.w1, s.omw1 = r.omw1, s.beta2 = r.beta2, s.w2 = r.w2;
        s.sqrt_bc2 = r.sqrt_bc2, s.nstep = r.nstep, s.eps = r.eps;
        const bool use_p = s.decay || s.adam, use_g = s.clip || s.adam, use_mv = s.adam;
        const int64_t start = (int64_t)a.c_index[c] * TTS_OPTIM_CHUNK;
        const int64_t left = r.numel - start;
        const int cnt = left < TTS_OPTIM_CHUNK ? (int)left : TTS_OPTIM_CHUNK;
        float* p = r.p + start;
        float* g = use_g ? r.g + start : nullptr;
        float* m = use_mv ? r.m + start : nullptr;
        float* v = use_mv ? r.v + start : nullptr;
        uintptr_t bits = 0;  // (a null pointer is aligned)
        if (use_p) bits |= reinterpret_cast<uintptr_t>(p);
        bits |= reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
        const bool vec = (bits & 15) == 0;
#pragma unroll 2
        for (int j = 0; j < OPT_QUADS; ++j) {
            const int e = 4 * (tid + j * OPT_THREADS);
            if (e >= cnt) break;
            if (vec && e + 4 <= cnt) {
                float4a P = {0.f, 0.f, 0.f, 0.f}, G = P, M = P, V = P;
                if (use_p) P = ld4(p + e);
                if (use_g) G = ld4(g + e);
                if (use_mv) {
                    M = ld4(m + e);
                    V = ld4(v + e);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pp = P[k], gg = G[k], mm = M[k], vv = V[k];
                    update_element(s, pp, gg, mm, vv);
                    P[k] = pp, G[k] = gg, M[k] = mm, V[k] = vv;
                }
                if (use_p) st4(p + e, P);
                if (s.clip) st4(g + e, G);
                if (use_mv) {
                    st4(m + e, M);
                    st4(v + e, V);
                }
            } else {
                for (int k = 0; k < 4 && e + k < cnt; ++k) {
                    const int i = e + k;
                    float pp = use_p ? ld1(p + i) : 0.f, gg = use_g ? ld1(g + i) : 0.f;
                    float mm = use_mv ? ld1(m + i) : 0.f, vv = use_mv ? ld1(v + i) : 0.f;
                    update_element(s, pp, gg, mm, vv);
                    if (use_p) st1(p + i, pp);
                    if (s.clip) st1(g + i, gg);
                    if (use_mv) {
                        st1(m + i, mm);
                        st1(v + i, vv);
                    }
                }
            }
        }
    }
}

}  // namespace
}  // namespace tts

// The chunk map of the current sizes (device), the partials, the device copy of the per-call table and
// OPT_RING pinned host copies of it, each with the event that says the stream has read it.
struct tts_optim {
    std::vector<int64_t> numel;
    int chunks = 0;
    tts::DeviceBuf<char> dev;
    size_t off_rows = 0, off_tensor = 0, off_index = 0;
    std::vector<int> host_map;
    tts::Row* pinned[tts::OPT_RING] = {};
    hipEvent_t read[tts::OPT_RING] = {};
    bool pending[tts::OPT_RING] = {};
    int next = 0;
};

namespace tts {
namespace {

void free_pinned(tts_optim* o) {
    for (int i = 0; i < OPT_RING; ++i) {
        if (o->pending[i]) (void)hipEventSynchronize(o->read[i]);
        if (o->pinned[i]) (void)hipHostFree(o->pinned[i]);
        o->pinned[i] = nullptr;
        o->pending[i] = false;
    }
}

struct Hyper {
    double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0, wd = 0.0;
};

// The checks every entry point shares.  state: a tensor with a gradient needs m, v and a step >= 1.
tts_status check_table(const tts_optim* o, const tts_optim_tensor* t, int n, bool state, const char* who) {
    const std::string w(who);
    TTS_CHECK(o && t, TTS_ERR_INVALID, w + ": null argument");
    TTS_CHECK(n > 0, TTS_ERR_INVALID, w + ": n must be positive");
    TTS_CHECK(!o->numel.empty(), TTS_ERR_INVALID, w + ": tts_optim_set_tensors has not been called");
    TTS_CHECK((size_t)n == o->numel.size(), TTS_ERR_INVALID,
              w + ": " + std::to_string(n) + " tensors, the sizes were set for " + std::to_string(o->numel.size()));
    std::vector<const float*> seen(n);
    for (int i = 0; i < n; ++i) {
        TTS_CHECK(t[i].numel > 0, TTS_ERR_INVALID, w + ": tensor " + std::to_string(i) + " has no positive element count");
        TTS_CHECK(t[i].numel == o->numel[i], TTS_ERR_INVALID,
                  w + ": tensor " + std::to_string(i) + " has " + std::to_string(t[i].numel) +
                      " elements, the sizes were set for " + std::to_string(o->numel[i]));
        TTS_CHECK(t[i].p, TTS_ERR_INVALID, w + ": tensor " + std::to_string(i) + " has a null p");
        TTS_CHECK(!state || !t[i].g || (t[i].m && t[i].v), TTS_ERR_INVALID,
                  w + ": tensor " + std::to_string(i) + " has a null m or v");
        TTS_CHECK(!state || !t[i].g || t[i].step >= 1, TTS_ERR_INVALID,
                  w + ": tensor " + std::to_string(i) + " has a step below 1");
        seen[i] = t[i].p;
    }
    std::sort(seen.begin(), seen.end());
    TTS_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), TTS_ERR_INVALID,
              w + ": two tensors have the same p");
    return TTS_OK;
}

tts_status check_hyper(const Hyper& h, bool adam, const char* who) {
    const std::string w(who);
    TTS_CHECK(h.lr > 0.0, TTS_ERR_INVALID, w + ": lr must be positive");
    if (!adam) return TTS_OK;
    TTS_CHECK(h.beta1 >= 0.0 && h.beta1 < 1.0 && h.beta2 >= 0.0 && h.beta2 < 1.0, TTS_ERR_INVALID,
              w + ": a beta is outside [0, 1)");
    TTS_CHECK(h.eps >= 0.0, TTS_ERR_INVALID, w + ": eps is negative");
    return TTS_OK;
}

// Fills the next pinned copy of the table and enqueues its upload.
tts_status upload(tts_optim* o, const tts_optim_tensor* t, int n, const Hyper& h, bool adam, hipStream_t s) {
    const int slot = o->next;
    if (o->pending[slot]) TTS_HIP(hipEventSynchronize(o->read[slot]));
    o->pending[slot] = false;
    Row* rows = o->pinned[slot];
    for (int i = 0; i < n; ++i) {
        Row& r = rows[i];
        r.p = t[i].p, r.g = t[i].g, r.m = t[i].m, r.v = t[i].v, r.numel = t[i].numel;
        r.dlr = (float)(-h.wd * h.lr);
        r.w1 = r.omw1 = r.beta2 = r.w2 = r.sqrt_bc2 = r.nstep = r.eps = 0.f;
        if (adam && t[i].g) {  // torch/optim/adam.py, _single_tensor_adam: Python doubles, rounded as the scalars of the ops are
            const double step = (double)t[i].step;
            const double bc1 = 1.0 - std::pow(h.beta1, step), bc2 = 1.0 - std::pow(h.beta2, step);
            r.w1 = (float)(1.0 - h.beta1);
            r.omw1 = 1.0f - r.w1;
            r.beta2 = (float)h.beta2;
            r.w2 = (float)(1.0 - h.beta2);
            r.sqrt_bc2 = (float)std::sqrt(bc2);
            r.nstep = (float)(-(h.lr / bc1));
            r.eps = (float)h.eps;
        }
    }
    TTS_HIP(hipMemcpyAsync(o->dev.p + o->off_rows, rows, (size_t)n * sizeof(Row), hipMemcpyHostToDevice, s));
    TTS_HIP(hipEventRecord(o->read[slot], s));
    o->pending[slot] = true;
    o->next = (slot + 1) % OPT_RING;
    return TTS_OK;
}

inline const Row* dev_rows(const tts_optim* o) { return reinterpret_cast<const Row*>(o->dev.p + o->off_rows); }
inline const int* dev_tensor(const tts_optim* o) { return reinterpret_cast<const int*>(o->dev.p + o->off_tensor); }
inline const int* dev_index(const tts_optim* o) { return reinterpret_cast<const int*>(o->dev.p + o->off_index); }

tts_status launch_norm(tts_optim* o, double max_norm, double* norm64, float* norm32, hipStream_t s) {
    double* partial = reinterpret_cast<double*>(o->dev.p);
    const NormArgs a{dev_rows(o), dev_tensor(o), dev_index(o), o->chunks, partial};
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(std::min(o->chunks, OPT_MAX_GRID)), dim3(OPT_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    const FoldArgs f{partial, o->chunks, max_norm, norm64, norm32};
    hipLaunchKernelGGL(optim_fold_kernel, dim3(1), dim3(OPT_FOLD_THREADS), 0, s, f);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status launch_update(tts_optim* o, int flags, const float* coef, hipStream_t s) {
    const UpdateArgs a{dev_rows(o), dev_tensor(o), dev_index(o), o->chunks, flags, coef};
    hipLaunchKernelGGL(optim_update_kernel, dim3(std::min(o->chunks, OPT_MAX_GRID)), dim3(OPT_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

tts_status norm_to_host(const double* norm64, double* sumsq_out, double* norm_out, hipStream_t s) {
    if (!sumsq_out && !norm_out) return TTS_OK;
    double back[2];
    TTS_HIP(hipMemcpyAsync(back, norm64, sizeof(back), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipStreamSynchronize(s));
    if (sumsq_out) *sumsq_out = back[0];
    if (norm_out) *norm_out = back[1];
    return TTS_OK;
}

}  // namespace
}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_optim_create(tts_optim** out) {
    TTS_CHECK(out, TTS_ERR_INVALID, "optim_create: null argument");
    tts_optim* o = new tts_optim();
    for (int i = 0; i < OPT_RING; ++i) {
        const hipError_t e = hipEventCreateWithFlags(&o->read[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            tts_optim_destroy(o);
            TTS_HIP(e);
        }
    }
    *out = o;
    return TTS_OK;
}

void tts_optim_destroy(tts_optim* o) {
    if (!o) return;
    free_pinned(o);
    for (int i = 0; i < OPT_RING; ++i)
        if (o->read[i]) (void)hipEventDestroy(o->read[i]);
    if (o->dev.p) (void)hipFree(o->dev.p);
    delete o;
}

tts_status tts_optim_set_tensors(tts_optim* o, const int64_t* numel, int n, void* stream) {
    TTS_CHECK(o && numel, TTS_ERR_INVALID, "optim_set_tensors: null argument");
    TTS_CHECK(n > 0, TTS_ERR_INVALID, "optim_set_tensors: n must be positive");
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        TTS_CHECK(numel[i] > 0, TTS_ERR_INVALID,
                  "optim_set_tensors: tensor " + std::to_string(i) + " has no positive element count");
        chunks += (numel[i] + TTS_OPTIM_CHUNK - 1) / TTS_OPTIM_CHUNK;
        TTS_CHECK(chunks <= INT32_MAX, TTS_ERR_INVALID, "optim_set_tensors: more than 2^31 - 1 chunks of work");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TTS_HIP(hipStreamSynchronize(s));  // an earlier call may still read the map and the table
    free_pinned(o);
    o->numel.clear();  // (not set, should anything below fail)
    o->host_map.resize(2 * (size_t)chunks);
    int c = 0;
    for (int i = 0; i < n; ++i)
        for (int64_t k = 0; k < (numel[i] + TTS_OPTIM_CHUNK - 1) / TTS_OPTIM_CHUNK; ++k, ++c) {
            o->host_map[c] = i;
            o->host_map[(size_t)chunks + c] = (int)k;
        }
    // [chunks] partials, [n] rows, [chunks] tensor, [chunks] index
    o->off_rows = (size_t)chunks * sizeof(double);
    o->off_tensor = o->off_rows + (size_t)n * sizeof(Row);
    o->off_index = o->off_tensor + (size_t)chunks * sizeof(int);
    TTS_TRY(o->dev.reserve(o->off_index + (size_t)chunks * sizeof(int)));
    TTS_HIP(hipMemcpyAsync(o->dev.p + o->off_tensor, o->host_map.data(), 2 * (size_t)chunks * sizeof(int),
                           hipMemcpyHostToDevice, s));
    TTS_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < OPT_RING; ++i)
        TTS_HIP(hipHostMalloc(reinterpret_cast<void**>(&o->pinned[i]), (size_t)n * sizeof(Row), hipHostMallocDefault));
    o->next = 0;
    o->chunks = (int)chunks;
    o->numel.assign(numel, numel + n);
    return TTS_OK;
}

tts_status tts_optim_grad_norm(tts_optim* o, const tts_optim_tensor* t, int n, double max_norm, double* norm64_dev,
                               float* norm32_dev, double* sumsq_out, double* norm_out, void* stream) {
    TTS_TRY(check_table(o, t, n, false, "optim_grad_norm"));
    TTS_CHECK(norm64_dev && norm32_dev, TTS_ERR_INVALID, "optim_grad_norm: null argument");
    TTS_CHECK(max_norm > 0.0, TTS_ERR_INVALID, "optim_grad_norm: max_norm must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TTS_TRY(upload(o, t, n, Hyper(), false, s));
    TTS_TRY(launch_norm(o, max_norm, norm64_dev, norm32_dev, s));
    return norm_to_host(norm64_dev, sumsq_out, norm_out, s);
}

tts_status tts_optim_clip(tts_optim* o, const tts_optim_tensor* t, int n, double max_norm, double* norm64_dev,
                          float* norm32_dev, double* sumsq_out, double* norm_out, void* stream) {
    TTS_TRY(check_table(o, t, n, false, "optim_clip"));
    TTS_CHECK(norm64_dev && norm32_dev, TTS_ERR_INVALID, "optim_clip: null argument");
    TTS_CHECK(max_norm > 0.0, TTS_ERR_INVALID, "optim_clip: max_norm must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TTS_TRY(upload(o, t, n, Hyper(), false, s));
    TTS_TRY(launch_norm(o, max_norm, norm64_dev, norm32_dev, s));
    TTS_TRY(launch_update(o, F_CLIP, norm32_dev + 1, s));
    return norm_to_host(norm64_dev, sumsq_out, norm_out, s);
}

tts_status tts_optim_decay(tts_optim* o, const tts_optim_tensor* t, int n, double lr, double wd, void* stream) {
    TTS_TRY(check_table(o, t, n, false, "optim_decay"));
    Hyper h;
    h.lr = lr, h.wd = wd;
    TTS_TRY(check_hyper(h, false, "optim_decay"));
    if (wd == 0.0) return TTS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TTS_TRY(upload(o, t, n, h, false, s));
    return launch_update(o, F_DECAY, nullptr, s);
}

tts_status tts_optim_adam(tts_optim* o, const tts_optim_tensor* t, int n, double lr, double beta1, double beta2,
                          double eps, void* stream) {
    TTS_TRY(check_table(o, t, n, true, "optim_adam"));
    Hyper h;
    h.lr = lr, h.beta1 = beta1, h.beta2 = beta2, h.eps = eps;
    TTS_TRY(check_hyper(h, true, "optim_adam"));
    hipStream_t s = static_cast<hipStream_t>(stream);
    TTS_TRY(upload(o, t, n, h, true, s));
    return launch_update(o, F_ADAM, nullptr, s);
}

tts_status tts_optim_step(tts_optim* o, const tts_optim_tensor* t, int n, double lr, double beta1, double beta2,
                          double eps, double wd, double max_norm, double* norm64_dev, float* norm32_dev,
                          void* stream) {
    TTS_TRY(check_table(o, t, n, true, "optim_step"));
    TTS_CHECK(norm64_dev && norm32_dev, TTS_ERR_INVALID, "optim_step: null argument");
    Hyper h;
    h.lr = lr, h.beta1 = beta1, h.beta2 = beta2, h.eps = eps, h.wd = wd;
    TTS_TRY(check_hyper(h, true, "optim_step"));
    TTS_CHECK(max_norm > 0.0, TTS_ERR_INVALID, "optim_step: max_norm must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TTS_TRY(upload(o, t, n, h, true, s));
    TTS_TRY(launch_norm(o, max_norm, norm64_dev, norm32_dev, s));
    return launch_update(o, (wd != 0.0 ? F_DECAY : 0) | F_CLIP | F_ADAM, norm32_dev + 1, s);
}

}  // extern "C"
