// The analysis half of AudioProcessor on the device, on the Griffin-Lim handle's tables and
// stream: spectrogram / melspectrogram of waveforms, and a model's linear output to mel.
#include <cmath>
#include <vector>

#include "gl_fft.h"

using namespace tts;

namespace {

// AudioProcessor.spectrogram and .melspectrogram (utils/audio.py:138-152) from one STFT, as
// collate_fn computes them for every wav (datasets/TTSDataset.py:191-192) and compute_style_mel
// for the GST style wav (utils/synthesis.py:28-35): pre-emphasis FIR (lfilter([1, -c], [1]),
// :128-131) -> librosa 0.6.2 stft (centre reflect pad, periodic Hann, float64 FFT, complex64
// result) -> |D| (float32), then
//   linear: 20 log10(max(min_level, |D|)) - ref_level_db -> _normalize (:79-94)
//   mel:    mel_basis . |D| (float64) -> the same two steps.
// One workgroup per (sentence, frame); outputs frame-major [B][Fmax][1025] and [B][Fmax][num_mels]
// float32, rows at and beyond a sentence's frame count zero.
struct NormArgs {
    double min_level, min_db, ref_db, max_norm;
    int signal_norm, symmetric, clip;
};

// _amp_to_db(x) - ref_level_db -> _normalize (utils/audio.py:121-123, :79-94), float64
__device__ __forceinline__ double amp_to_norm_db(double x, const NormArgs& n) {
    double S = 20.0 * log10(fmax(n.min_level, x)) - n.ref_db;
    if (n.signal_norm) {
        S = (S - n.min_db) / -n.min_db;
        if (n.symmetric) {
            S = (2.0 * n.max_norm) * S - n.max_norm;
            if (n.clip) S = fmin(fmax(S, -n.max_norm), n.max_norm);
        } else {
            S = n.max_norm * S;
            if (n.clip) S = fmin(fmax(S, 0.0), n.max_norm);
        }
    }
    return S;
}

struct MelArgs {
    const double* wav;  // [B][Nmax]
    int64_t Nmax;
    const int* N;       // [B] samples
    int Fmax;
    Geo g;
    GLConst c;
    const double* basis;  // [num_mels][1025]
    int n_mels;
    double coef;          // pre-emphasis (0: none)
    NormArgs n;
    float* lin;           // [B][Fmax][1025] (LIN)
    float* mel;           // [B][Fmax][n_mels] (MEL)
};

template <bool LIN, bool MEL>
__global__ __launch_bounds__(GL_THREADS) void analysis_kernel(const MelArgs a) {
    const int b = blockIdx.y, f = blockIdx.x;
    const int N = a.N[b];
    const int F = 1 + N / a.g.hop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)b * a.Fmax + f;
    if (f >= F) {  // padding row
        if (LIN)
            for (int k = tid; k < NB; k += GL_THREADS) a.lin[row * NB + k] = 0.f;
        if (MEL)
            for (int m = tid; m < a.n_mels; m += GL_THREADS) a.mel[row * a.n_mels + m] = 0.f;
        return;
    }
    __shared__ __align__(16) double2 buf0[NH];
    __shared__ __align__(16) double2 buf1[NH];
    __shared__ float mag[MEL ? NB + 3 : 1];
    const FftTw ftw = load_fft_tw(a.c.tw);
    const double* y = a.wav + (int64_t)b * a.Nmax;
    constexpr int PN = NFFT / GL_THREADS;
    double* xr = reinterpret_cast<double*>(buf0);
#pragma unroll
    for (int i = 0; i < PN; ++i) {
        const int n = tid + i * GL_THREADS;
        // np.pad(y_pre, n_fft // 2, mode='reflect') of the pre-emphasised signal
        const int p = reflect_idx(f * a.g.hop + n - NFFT / 2, N);
        double v = y[p];
        if (a.coef != 0.0 && p > 0) v = v - a.coef * y[p - 1];
        xr[n] = a.c.win[n] * v;
    }
    __syncthreads();
    const double2* Z = fft1024<false>(buf0, buf1, ftw);
    for (int k = tid; k < NB; k += GL_THREADS) {
        const double2 zk = Z[k & (NH - 1)];
        const double2 zc = cconj(Z[(NH - k) & (NH - 1)]);
        const double2 E = double2{0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y)};
        const double2 O = double2{0.5 * (zk.y - zc.y), -0.5 * (zk.x - zc.x)};
        const double2 t = a.c.tw[k];
        const float re = (float)(E.x + (t.x * O.x - t.y * O.y));  // stft result is complex64
        const float im = (float)(E.y + (t.x * O.y + t.y * O.x));
        const float mk = hypotf(re, im);  // np.abs on complex64
        if (MEL) mag[k] = mk;
        // utils/audio.py:143-144; the float64 min_level promotes the float32 magnitude
        if (LIN) a.lin[row * NB + k] = (float)amp_to_norm_db((double)mk, a.n);
    }
    if (!MEL) return;
    __syncthreads();
    // mel bands: each wave owns bands wave, wave+4, ...; lanes stride the 1025 bins, float64
    for (int m = wave; m < a.n_mels; m += GL_THREADS / 64) {
        const double* brow = a.basis + (int64_t)m * NB;
        double acc = 0.0;
        for (int k = lane; k < NB; k += 64) acc += brow[k] * (double)mag[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) a.mel[row * a.n_mels + m] = (float)amp_to_norm_db(acc, a.n);
    }
}

// ---------------------------------------------------------------- linear -> mel
// AudioProcessor.out_linear_to_mel (utils/audio.py:174-180) on a model's linear output:
// _denormalize -> + ref_level_db -> 10^(x * 0.05) (float32, as numpy keeps them for a float32
// input) -> mel_basis . S (float64) -> _amp_to_db - ref_level_db -> _normalize.
// A workgroup takes L2M_TF consecutive frames of one sentence: their values become amplitudes once,
// in LDS, and each thread then owns (band, frame) pairs and sums only the band's nonzero bins
// [band[2m], band[2m+1]) (a Slaney triangle covers a short run of bins; the exact zeros outside it
// add nothing).  Bins outside [k_lo, k_hi), the union of the bands (above mel_fmax, below mel_fmin),
// feed no band and are neither read nor converted.  The tile's loads are all issued before the first
// conversion.  The frame is the fast index of a pair, so a wave's lanes walk bands of similar
// length, and the rows' odd pitch (1025 floats) spreads the frames over the LDS banks.
#ifndef TTS_L2M_TF  // frames per workgroup; -DTTS_L2M_TF=n builds the variants of DESIGN 4's sweep (4 won)
#define TTS_L2M_TF 4
#endif
constexpr int L2M_TF = TTS_L2M_TF;
constexpr int L2M_THREADS = 256;
constexpr int L2M_PER = (NB + L2M_THREADS - 1) / L2M_THREADS;  // bins of a row per thread

struct L2MArgs {
    const float* lin;  // [B][Fmax][1025]
    const int* F;      // [B] frames
    int Fmax;
    const double* basis;  // [num_mels][1025]
    const int* band;      // [num_mels][2]: first nonzero bin, one past the last
    int k_lo, k_hi;       // the bands' union
    int n_mels;
    float min_db, ref_db, max_norm;  // the float32 side (_denormalize, dB -> amplitude)
    NormArgs n;
    float* mel;  // [B][Fmax][n_mels]
};

__global__ __launch_bounds__(L2M_THREADS) void linear_to_mel_kernel(const L2MArgs a) {
    const int b = blockIdx.y, f0 = blockIdx.x * L2M_TF;
    const int tid = threadIdx.x;
    const int F = a.F[b];
    const int nf = min(L2M_TF, F - f0);              // frames of the sentence in this tile (may be <= 0)
    const int nt = min(L2M_TF, a.Fmax - f0);         // rows of the tile
    const int64_t row0 = (int64_t)b * a.Fmax + f0;
    for (int i = max(nf, 0) * a.n_mels + tid; i < nt * a.n_mels; i += L2M_THREADS) a.mel[row0 * a.n_mels + i] = 0.f;
    if (nf <= 0) return;
    __shared__ float amp[L2M_TF * NB];
    const float* src = a.lin + row0 * NB;
    float v[L2M_TF][L2M_PER];
#pragma unroll
    for (int fl = 0; fl < L2M_TF; ++fl)
#pragma unroll
        for (int j = 0; j < L2M_PER; ++j) {
            const int k = a.k_lo + tid + j * L2M_THREADS;
            v[fl][j] = fl < nf && k < a.k_hi ? src[fl * NB + k] : 0.f;
        }
#pragma unroll
    for (int fl = 0; fl < L2M_TF; ++fl)
#pragma unroll
        for (int j = 0; j < L2M_PER; ++j) {
            const int k = a.k_lo + tid + j * L2M_THREADS;
            if (fl >= nf || k >= a.k_hi) continue;
            float S = v[fl][j];
            if (a.n.signal_norm) {  // utils/audio.py:96-112
                if (a.n.symmetric) {
                    if (a.n.clip) S = fminf(fmaxf(S, -a.max_norm), a.max_norm);
                    S = ((S + a.max_norm) * -a.min_db / (2.f * a.max_norm)) + a.min_db;
                } else {
                    if (a.n.clip) S = fminf(fmaxf(S, 0.f), a.max_norm);
                    S = (S * -a.min_db / a.max_norm) + a.min_db;
                }
            }
            amp[fl * NB + k] = exp10f((S + a.ref_db) * 0.05f);  // utils/audio.py:176, :125-126
        }
    __syncthreads();
    for (int p = tid; p < a.n_mels * L2M_TF; p += L2M_THREADS) {
        const int m = p / L2M_TF, fl = p % L2M_TF;
        if (fl >= nf) continue;
        const int k0 = a.band[2 * m], k1 = a.band[2 * m + 1];
        const double* brow = a.basis + (int64_t)m * NB;
        const float* x = amp + fl * NB;
        double acc = 0.0;
#pragma unroll 8  // eight basis loads in flight; the sum keeps its order
        for (int k = k0; k < k1; ++k) acc += brow[k] * (double)x[k];
        a.mel[(row0 + fl) * a.n_mels + m] = (float)amp_to_norm_db(acc, a.n);
    }
}

// the per-sentence counts of an analysis / conversion call, on the device (g->stream)
tts_status upload_counts(tts_gl* g, const int32_t* v, int B, hipStream_t s) {
    if ((size_t)B > g->NS.cap) TTS_HIP(hipStreamSynchronize(s));
    TTS_TRY(g->NS.reserve(B));
    TTS_HIP(hipMemcpyAsync(g->NS.p, v, B * sizeof(int), hipMemcpyHostToDevice, s));
    return TTS_OK;
}

NormArgs norm_args(const tts_audio_config& c) {
    NormArgs n{};
    n.min_db = c.min_level_db;
    n.min_level = std::exp((double)c.min_level_db / 20.0 * std::log(10.0));  // utils/audio.py:122
    n.ref_db = c.ref_level_db;
    n.max_norm = c.max_norm;
    n.signal_norm = c.signal_norm;
    n.symmetric = c.symmetric_norm;
    n.clip = c.clip_norm;
    return n;
}

// tts_gl_analyze / tts_gl_melspectrogram: one launch, one FFT per frame, either or both outputs
tts_status gl_analyze(tts_gl* g, const double* wav, const int32_t* N, int B, int64_t Nmax, float* lin, float* mel,
                      int Fmax, void* stream) {
    TTS_CHECK(g && wav && N && B >= 1 && Fmax >= 1, TTS_ERR_INVALID, "bad analysis arguments");
    TTS_CHECK(lin || mel, TTS_ERR_INVALID, "analysis needs at least one output");
    TTS_CHECK(!mel || g->basis, TTS_ERR_INVALID, "mel analysis needs tts_gl_set_mel_basis first");
    TTS_CHECK(B <= 65535, TTS_ERR_INVALID, "B > 65535");
    for (int b = 0; b < B; ++b) {
        TTS_CHECK(N[b] >= 2 && N[b] <= Nmax, TTS_ERR_INVALID, "N[b] out of range [2, Nmax]");
        TTS_CHECK(1 + N[b] / g->g.hop <= Fmax, TTS_ERR_INVALID, "Fmax < 1 + N[b] / hop");
    }
    hipStream_t cs = static_cast<hipStream_t>(stream);
    hipStream_t s = g->stream;
    TTS_HIP(hipEventRecord(g->ev_in, cs));
    TTS_HIP(hipStreamWaitEvent(s, g->ev_in, 0));
    TTS_TRY(upload_counts(g, N, B, s));
    MelArgs a{};
    a.wav = wav;
    a.Nmax = Nmax;
    a.N = g->NS.p;
    a.Fmax = Fmax;
    a.g = g->g;
    a.c = GLConst{g->win, g->win2, g->tw};
    a.basis = g->basis;
    a.n_mels = g->cfg.num_mels;
    a.coef = g->cfg.preemphasis;
    a.n = norm_args(g->cfg);
    a.lin = lin;
    a.mel = mel;
    const dim3 grid(Fmax, B), block(GL_THREADS);
    if (lin && mel)
        hipLaunchKernelGGL((analysis_kernel<true, true>), grid, block, 0, s, a);
    else if (lin)
        hipLaunchKernelGGL((analysis_kernel<true, false>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((analysis_kernel<false, true>), grid, block, 0, s, a);
    TTS_HIP(hipGetLastError());
    TTS_HIP(hipEventRecord(g->ev_out, s));
    TTS_HIP(hipStreamWaitEvent(cs, g->ev_out, 0));
    return TTS_OK;
}

}  // namespace

extern "C" {

tts_status tts_gl_set_mel_basis(tts_gl* g, const double* mel_basis) {
    TTS_CHECK(g && mel_basis, TTS_ERR_INVALID, "null argument");
    const int M = g->cfg.num_mels;
    const size_t n = (size_t)M * NB;
    // each row's nonzero bins [first, last): linear_to_mel_kernel sums only inside them
    std::vector<int> band(2 * (size_t)M, 0);
    int lo = NB, hi = 0;
    for (int m = 0; m < M; ++m) {
        const double* row = mel_basis + (size_t)m * NB;
        int k0 = 0, k1 = NB;
        while (k0 < NB && row[k0] == 0.0) ++k0;
        while (k1 > k0 && row[k1 - 1] == 0.0) --k1;
        if (k0 == NB) continue;  // an empty filter
        band[2 * m] = k0;
        band[2 * m + 1] = k1;
        lo = std::min(lo, k0);
        hi = std::max(hi, k1);
    }
    if (!g->band) TTS_HIP(hipMalloc(&g->band, band.size() * sizeof(int)));
    if (!g->basis) TTS_HIP(hipMalloc(&g->basis, n * sizeof(double)));
    TTS_HIP(hipStreamSynchronize(g->stream));  // a conversion still reading the previous basis
    TTS_HIP(hipMemcpy(g->band, band.data(), band.size() * sizeof(int), hipMemcpyHostToDevice));
    TTS_HIP(hipMemcpy(g->basis, mel_basis, n * sizeof(double), hipMemcpyHostToDevice));
    g->band_lo = std::min(lo, hi);
    g->band_hi = hi;
    return TTS_OK;
}

tts_status tts_gl_melspectrogram(tts_gl* g, const double* wav, const int32_t* N, int B, int64_t Nmax, float* mel,
                                 int Fmax, void* stream) {
    TTS_CHECK(mel, TTS_ERR_INVALID, "bad melspectrogram arguments");
    return gl_analyze(g, wav, N, B, Nmax, nullptr, mel, Fmax, stream);
}

tts_status tts_gl_analyze(tts_gl* g, const double* wav, const int32_t* N, int B, int64_t Nmax, float* linear,
                          float* mel, int Fmax, void* stream) {
    return gl_analyze(g, wav, N, B, Nmax, linear, mel, Fmax, stream);
}

tts_status tts_gl_linear_to_mel(tts_gl* g, const float* linear, const int32_t* F, int B, int Fmax, float* mel,
                                void* stream) {
    TTS_CHECK(g && linear && F && mel && B >= 1 && Fmax >= 1, TTS_ERR_INVALID, "bad linear_to_mel arguments");
    TTS_CHECK(g->basis && g->band, TTS_ERR_INVALID, "tts_gl_linear_to_mel needs tts_gl_set_mel_basis first");
    TTS_CHECK(B <= 65535, TTS_ERR_INVALID, "B > 65535");
    for (int b = 0; b < B; ++b) TTS_CHECK(F[b] >= 1 && F[b] <= Fmax, TTS_ERR_INVALID, "F[b] out of range [1, Fmax]");
    hipStream_t cs = static_cast<hipStream_t>(stream);
    hipStream_t s = g->stream;
    TTS_HIP(hipEventRecord(g->ev_in, cs));
    TTS_HIP(hipStreamWaitEvent(s, g->ev_in, 0));
    TTS_TRY(upload_counts(g, F, B, s));
    L2MArgs a{};
    a.lin = linear;
    a.F = g->NS.p;
    a.Fmax = Fmax;
    a.basis = g->basis;
    a.band = g->band;
    a.k_lo = g->band_lo;
    a.k_hi = g->band_hi;
    a.n_mels = g->cfg.num_mels;
    a.min_db = g->cfg.min_level_db;
    a.ref_db = g->cfg.ref_level_db;
    a.max_norm = g->cfg.max_norm;
    a.n = norm_args(g->cfg);
    a.mel = mel;
    hipLaunchKernelGGL(linear_to_mel_kernel, dim3((Fmax + L2M_TF - 1) / L2M_TF, B), dim3(L2M_THREADS), 0, s, a);
    TTS_HIP(hipGetLastError());
    TTS_HIP(hipEventRecord(g->ev_out, s));
    TTS_HIP(hipStreamWaitEvent(cs, g->ev_out, 0));
    return TTS_OK;
}

}  // extern "C"
