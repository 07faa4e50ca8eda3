// The reference's silence handling on ragged batches in HBM:
//   AudioProcessor.trim_silence (utils/audio.py:212-217): drop a margin on both sides, then librosa 0.6.2
//     effects.trim: mean square of centre-padded (reflect) frames, 10 log10 against the loudest frame,
//     keep what lies between the first and the last frame above -top_db;
//   AudioProcessor.find_endpoint (utils/audio.py:203-210): the first window, stepped by a hop, whose
//     SIGNED maximum lies strictly below a threshold;
//   a segment gather that hands the kept stretch of every sentence to the analysis entry points.
// Each of the two searches is two launches: one value per frame (a wave per frame, one fixed summation
// order: lane l adds samples l, l + 64, ... in index order, then a 6-level xor butterfly over the lanes,
// every lane the same total) or per candidate window (a workgroup per window; a maximum rounds nothing),
// then one workgroup per sentence over those values.  No sample at or beyond N[b] is read: the reflect
// padding is index arithmetic on the sentence's own samples, and the last candidate window ends below
// N[b].  Integers out; nothing here depends on the order workgroups run in.
#include <cmath>

#include "gl_handle.h"

namespace tts {
namespace {

constexpr int SIL_THREADS = 256;
constexpr int SIL_WAVES = SIL_THREADS / WAVE;

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
    return v;
}

struct TrimArgs {
    const double* wav;
    int64_t pitch;
    const int* N;      // [B] samples per sentence
    int margin, frame_length, hop;
    double top_db;
    double* ms;        // [B][Fmax] mean square per frame
    int Fmax;
    int* out;          // [2][B] start, end
    int B;
};

// frame t of sentence b: frame_length samples centred on sample t * hop of the margin-stripped signal,
// reflect-padded (np.pad mode="reflect": index -i -> i, n - 1 + i -> n - 1 - i; n >= frame_length / 2 + 1
// makes one reflection enough, checked by the caller)
__global__ __launch_bounds__(SIL_THREADS) void trim_frames_kernel(const TrimArgs a) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1);
    const int t = blockIdx.x * SIL_WAVES + (threadIdx.x >> 6);
    const int n = a.N[b] - 2 * a.margin;
    if (t >= 1 + n / a.hop) return;  // (wave-uniform)
    const double* y = a.wav + (int64_t)b * a.pitch + a.margin;
    const int64_t first = (int64_t)t * a.hop - a.frame_length / 2;
    double s = 0.0;
    for (int j = lane; j < a.frame_length; j += WAVE) {
        int64_t i = first + j;
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (int64_t)(n - 1) - i;
        const double v = y[i];
        s += v * v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) a.ms[(int64_t)b * a.Fmax + t] = s / (double)a.frame_length;
}

// power_to_db against the loudest frame, the first and the last frame above -top_db
__global__ __launch_bounds__(SIL_THREADS) void trim_select_kernel(const TrimArgs a) {
    __shared__ double smax[SIL_WAVES];
    __shared__ int slo[SIL_WAVES], shi[SIL_WAVES];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const int n = a.N[b] - 2 * a.margin;
    const int F = 1 + n / a.hop;
    const double* ms = a.ms + (int64_t)b * a.Fmax;
    double m = 0.0;  // (mean squares are >= 0)
    for (int t = threadIdx.x; t < F; t += SIL_THREADS) m = fmax(m, ms[t]);
    m = wave_max_f64(m);
    if (lane == 0) smax[w] = m;
    __syncthreads();
    m = smax[0];
    for (int k = 1; k < SIL_WAVES; ++k) m = fmax(m, smax[k]);
    const double ref = 10.0 * log10(fmax(1e-10, m));
    int lo = F, hi = -1;
    for (int t = threadIdx.x; t < F; t += SIL_THREADS) {
        const double db = 10.0 * log10(fmax(1e-10, ms[t])) - ref;
        if (db > -a.top_db) {
            lo = min(lo, t);
            hi = max(hi, t);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, WAVE));
        hi = max(hi, __shfl_xor(hi, o, WAVE));
    }
    if (lane == 0) {
        slo[w] = lo;
        shi[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SIL_WAVES; ++k) {
            lo = min(lo, slo[k]);
            hi = max(hi, shi[k]);
        }
        // (nothing kept: the empty slice wav[0:0])
        a.out[b] = hi < 0 ? 0 : lo * a.hop;
        a.out[a.B + b] = hi < 0 ? 0 : (int)min((int64_t)n, (int64_t)(hi + 1) * a.hop);
    }
}

struct EndArgs {
    const double* wav;
    int64_t pitch;
    const int* N;
    int window, hop;
    double threshold;
    double* wmax;      // [B][Kmax] signed maximum of candidate k + 1's window
    int Kmax;
    int* out;          // [B]
};

// candidates x = k hop, k >= 1, x < N - window (Python's range: strict)
__device__ __forceinline__ int end_candidates(int N, int window, int hop) {
    return N - window > hop ? (N - window - 1) / hop : 0;
}

__global__ __launch_bounds__(SIL_THREADS) void end_window_kernel(const EndArgs a) {
    __shared__ double smax[SIL_WAVES];
    const int b = blockIdx.y, k = blockIdx.x;
    if (k >= end_candidates(a.N[b], a.window, a.hop)) return;  // (block-uniform)
    const double* y = a.wav + (int64_t)b * a.pitch + (int64_t)(k + 1) * a.hop;  // y[window - 1] lies below N[b]
    double m = -INFINITY;
    for (int j = threadIdx.x; j < a.window; j += SIL_THREADS) m = fmax(m, y[j]);
    m = wave_max_f64(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) smax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SIL_WAVES; ++w) m = fmax(m, smax[w]);
        a.wmax[(int64_t)b * a.Kmax + k] = m;
    }
}

__global__ __launch_bounds__(SIL_THREADS) void end_select_kernel(const EndArgs a) {
    __shared__ int sk[SIL_WAVES];
    const int b = blockIdx.x;
    const int K = end_candidates(a.N[b], a.window, a.hop);
    const double* wm = a.wmax + (int64_t)b * a.Kmax;
    int first = K;
    for (int k = threadIdx.x; k < K; k += SIL_THREADS)
        if (wm[k] < a.threshold) first = min(first, k);
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) sk[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SIL_WAVES; ++w) first = min(first, sk[w]);
        a.out[b] = first < K ? (first + 2) * a.hop : a.N[b];  // x + hop, x = (first + 1) hop
    }
}

struct SegArgs {
    const double* src;
    int64_t src_pitch;
    const int* seg;    // [2][B] start, len
    int B;
    double* dst;
    int64_t dst_pitch;
};

__global__ __launch_bounds__(SIL_THREADS) void take_segments_kernel(const SegArgs a) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * SIL_THREADS + threadIdx.x;
    if (i >= a.dst_pitch) return;
    const int start = a.seg[b], len = a.seg[a.B + b];
    a.dst[(int64_t)b * a.dst_pitch + i] = i < len ? a.src[(int64_t)b * a.src_pitch + start + i] : 0.0;
}

// the silence workspace: `values` doubles, then `ints` ints (grow only; idle whenever a call begins,
// since both calls that use it wait for their stream before they return)
tts_status silence_workspace(tts_gl* g, size_t values, size_t ints, double** v, int** i) {
    TTS_TRY(g->sil.reserve(values * sizeof(double) + ints * sizeof(int)));
    *v = reinterpret_cast<double*>(g->sil.p);
    *i = reinterpret_cast<int*>(*v + values);
    return TTS_OK;
}
}  // namespace

}  // namespace tts

using namespace tts;

extern "C" {

tts_status tts_gl_trim_silence(tts_gl* g, const double* wav, int64_t pitch, const int32_t* N, int B, int margin,
                               int frame_length, int hop_length, double top_db, int32_t* start_out,
                               int32_t* end_out, void* stream) {
    TTS_CHECK(g && wav && N && start_out && end_out, TTS_ERR_INVALID, "trim_silence: null argument");
    TTS_CHECK(B >= 1 && B <= 65535, TTS_ERR_INVALID, "trim_silence: B out of range [1, 65535]");
    TTS_CHECK(margin >= 0 && frame_length >= 2 && frame_length % 2 == 0 && hop_length >= 1, TTS_ERR_INVALID,
              "trim_silence: margin must be >= 0, frame_length positive and even, hop_length positive");
    int Fmax = 1;
    for (int b = 0; b < B; ++b) {
        TTS_CHECK(N[b] <= pitch, TTS_ERR_INVALID, "trim_silence: sentence " + std::to_string(b) + " has N[b] > pitch");
        TTS_CHECK(N[b] >= 2 * (int64_t)margin, TTS_ERR_INVALID,
                  "trim_silence: sentence " + std::to_string(b) + " is shorter than its two margins");
        const int n = N[b] - 2 * margin;
        TTS_CHECK(n >= frame_length / 2 + 1, TTS_ERR_INVALID,
                  "trim_silence: sentence " + std::to_string(b) + " has " + std::to_string(n) +
                      " samples between the margins, fewer than frame_length / 2 + 1 = " +
                      std::to_string(frame_length / 2 + 1) + " (the reflect padding needs one reflection)");
        Fmax = std::max(Fmax, 1 + n / hop_length);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* ms;
    int* iw;  // N [B], start [B], end [B]
    TTS_TRY(silence_workspace(g, (size_t)B * Fmax, (size_t)3 * B, &ms, &iw));
    TTS_HIP(hipMemcpyAsync(iw, N, B * sizeof(int), hipMemcpyHostToDevice, s));
    TrimArgs a{wav, pitch, iw, margin, frame_length, hop_length, top_db, ms, Fmax, iw + B, B};
    hipLaunchKernelGGL(trim_frames_kernel, dim3((Fmax + SIL_WAVES - 1) / SIL_WAVES, B), dim3(SIL_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    hipLaunchKernelGGL(trim_select_kernel, dim3(B), dim3(SIL_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    TTS_HIP(hipMemcpyAsync(start_out, iw + B, B * sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipMemcpyAsync(end_out, iw + 2 * B, B * sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipStreamSynchronize(s));
    return TTS_OK;
}

tts_status tts_gl_find_endpoint(tts_gl* g, const double* wav, int64_t pitch, const int32_t* N, int B,
                                int window_length, int hop_length, double threshold, int32_t* end_out,
                                void* stream) {
    TTS_CHECK(g && wav && N && end_out, TTS_ERR_INVALID, "find_endpoint: null argument");
    TTS_CHECK(B >= 1 && B <= 65535, TTS_ERR_INVALID, "find_endpoint: B out of range [1, 65535]");
    TTS_CHECK(window_length >= 1 && hop_length >= 1, TTS_ERR_INVALID,
              "find_endpoint: window_length and hop_length must be positive");
    int Kmax = 0;
    for (int b = 0; b < B; ++b) {
        TTS_CHECK(N[b] >= 0 && N[b] <= pitch, TTS_ERR_INVALID,
                  "find_endpoint: sentence " + std::to_string(b) + " has N[b] out of range [0, pitch]");
        // candidates x = k hop, k >= 1, x < N - window
        if ((int64_t)N[b] - window_length > hop_length)
            Kmax = std::max(Kmax, (N[b] - window_length - 1) / hop_length);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* wmax;
    int* iw;  // N [B], end [B]
    TTS_TRY(silence_workspace(g, (size_t)B * Kmax, (size_t)2 * B, &wmax, &iw));
    TTS_HIP(hipMemcpyAsync(iw, N, B * sizeof(int), hipMemcpyHostToDevice, s));
    EndArgs a{wav, pitch, iw, window_length, hop_length, threshold, wmax, Kmax, iw + B};
    if (Kmax > 0) {  // (0: no sentence has a candidate window)
        hipLaunchKernelGGL(end_window_kernel, dim3(Kmax, B), dim3(SIL_THREADS), 0, s, a);
        TTS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(end_select_kernel, dim3(B), dim3(SIL_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    TTS_HIP(hipMemcpyAsync(end_out, iw + B, B * sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP(hipStreamSynchronize(s));
    return TTS_OK;
}

tts_status tts_gl_take_segments(tts_gl* g, const double* src, int64_t src_pitch, const int32_t* start,
                                const int32_t* len, int B, double* dst, int64_t dst_pitch, void* stream) {
    TTS_CHECK(g && src && start && len && dst, TTS_ERR_INVALID, "take_segments: null argument");
    TTS_CHECK(B >= 1 && B <= 65535, TTS_ERR_INVALID, "take_segments: B out of range [1, 65535]");
    TTS_CHECK(dst_pitch >= 1 && dst_pitch <= INT32_MAX, TTS_ERR_INVALID, "take_segments: dst_pitch out of range");
    for (int b = 0; b < B; ++b) {
        TTS_CHECK(start[b] >= 0 && len[b] >= 0, TTS_ERR_INVALID,
                  "take_segments: sentence " + std::to_string(b) + " has a negative start or len");
        TTS_CHECK((int64_t)start[b] + len[b] <= src_pitch, TTS_ERR_INVALID,
                  "take_segments: sentence " + std::to_string(b) + " has start + len > src_pitch");
        TTS_CHECK(len[b] <= dst_pitch, TTS_ERR_INVALID,
                  "take_segments: sentence " + std::to_string(b) + " has len > dst_pitch");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (the previous gather on this stream may still read it)
    if ((size_t)2 * B > g->seg.cap) TTS_HIP(hipStreamSynchronize(s));
    TTS_TRY(g->seg.reserve(2 * B));
    g->seg_h.assign(start, start + B);
    g->seg_h.insert(g->seg_h.end(), len, len + B);
    TTS_HIP(hipMemcpyAsync(g->seg.p, g->seg_h.data(), 2 * B * sizeof(int), hipMemcpyHostToDevice, s));
    SegArgs a{src, src_pitch, g->seg.p, B, dst, dst_pitch};
    hipLaunchKernelGGL(take_segments_kernel, dim3((unsigned)((dst_pitch + SIL_THREADS - 1) / SIL_THREADS), B),
                       dim3(SIL_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    return TTS_OK;
}

}  // extern "C"
