// The Griffin-Lim / AudioProcessor handle (struct tts_gl), private to the files that implement
// its entry points: gl_handle.hip (create, destroy), griffin_lim.hip (synthesis), audio_analysis.hip
// (spectrogram, mel), phase_mt.hip (numpy-stream phases), wav_io.hip (PCM16 join), silence.hip,
// resample.hip.
#pragma once
#include <map>
#include <tuple>
#include <vector>

#include "host_util.h"

namespace tts {

typedef float spec_t;    // |S|^power storage
typedef float frame_t;   // windowed iSTFT frame storage (every loop: rounded once before librosa's
                         // float32 overlap-add, which adds each float64 frame into a float32 signal)
// the persistent loop's frame storage: one 8-byte granule per sample, {tag : 32 | float32 sample},
// the tag naming the iteration that wrote it (round 4; replaces float64 slots + per-frame flags)
struct gran_t {
    unsigned long long v;
};

constexpr int NFFT = 2048;
constexpr int NB = 1025;  // bins
constexpr int NH = 1024;  // complex FFT size
constexpr int GL_THREADS = 256;

struct Geo {
    int hop, win, woff, winp;  // woff = (NFFT - win) / 2, winp = win + (woff - fb) rounded up to 4
    int fb;                    // a frame slot holds samples [fb, fb + winp): fb = woff rounded down to
                               // even, so sample pairs (2n, 2n+1) are 16-byte aligned
};

struct GLConst {
    const double* win;    // [2048] padded periodic Hann
    const double* win2;   // [2048] win^2
    const double2* tw;    // [2048] e^{-2 pi i m / 2048}
};

// The launch arguments of an iteration and of the final overlap-add (griffin_lim.hip): the handle
// keeps the last run's for tts_gl_profile.
struct IterArgs {
    const spec_t* S;      // [B][Fmax][1025]
    const float* y;       // [B][Nmax] the previous iteration's float32 signal (gl_ola_kernel)
    const void* prev;     // FUSED: the previous iteration's frames (overlap-added here instead)
    int64_t Nmax;
    void* next;           // frames written by this iteration (frame_t; gran_t for the initial iSTFT of the persistent loop)
    const int* F;
    int Fmax;
    int B;
    Geo g;
    GLConst c;
    const double* phase_u;  // initial iSTFT only: [B][1025][Fmax] or null (device RNG)
    unsigned long long seed;
    unsigned* zero_flags;   // initial iSTFT only: the persistent loop's tag words to clear, or null
    int* zero_status;       // ... and its status word
    const double2* wt;      // gl_iter_wave_kernel: [16][4] pass-2 twiddles
    const double2* winc;    // gl_iter_wave_kernel: [4][64] window cosine seeds (see tts_gl_create)
    double wrot;            // ... and the recurrence factor 2 cos(2 pi 128 / win)
    unsigned gtag;          // initial iSTFT into granules (gran_t): the tag of iteration 0
};

struct FinArgs {
    const void* frames;  // frame_t (fused / batched loops) or gran_t (persistent): gl_ola_kernel<FT>
    const int* F;
    int Fmax, B;
    Geo g;
    GLConst c;
    float* y;  // [B][Nmax]
    int64_t Nmax;
    const int* status;  // the persistent loop's status word, or null: nonzero poisons the signal (NaN)
    int* host_status;   // pinned host word the status is copied to by thread 0 of block (0, 0), or null
    int* host_seq;      // ... then (pipeline mode) this pinned word is set to `seq` (release), or null
    int seq;
    const float* wssp;  // [hop] float32 window sum-square of a sample whose every contributing frame
                        // exists, by (q - woff) mod hop (summed on the host in ola_sample's order)
};

struct GraphKey {
    int B, Fmax, iters;
    bool operator<(const GraphKey& o) const { return std::tie(B, Fmax, iters) < std::tie(o.B, o.Fmax, o.iters); }
};

// phase_mt.hip: the device workspace of the numpy-stream draws (grown on demand; the caller orders reuse)
constexpr int MT_MAX_BATCH = 1024;
struct MtWork {
    unsigned* xs = nullptr;             // the raw word stream, [blocks][624]
    size_t xs_words = 0;
    unsigned long long* polys = nullptr;  // jump polynomials of chunks 1.., [n][312]
    int npolys = 0;
    long long* meta = nullptr;          // position, draws, last block, sentence offsets
};
void mt_work_free(MtWork* w);

// resample.hip: resampy's time register of one (orig_sr, target_sr) pair, tr[0] = 0, tr[t] = fl(tr[t - 1] + inc),
// summed serially on the host (grown on demand) and mirrored on the device
struct RsRegister {
    std::vector<double> host;
    DeviceBuf<double> dev;
    size_t uploaded = 0;  // leading values the device copy holds
};
// ... and one sentence of a resampling launch
struct RsSent {
    const double* tr;  // the pair's register on the device (null: pass-through)
    double scale;      // min(1, ratio)
    double mult;       // ratio when it is < 1, else 1: win[o] = half_win[o] * mult
    int N, n_res, step;
    int first;         // first workgroup of the sentence
};

}  // namespace tts

struct tts_gl {
    tts_audio_config cfg{};
    tts::Geo g{};
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    hipEvent_t ev_done = nullptr;  // end of the last tts_gl_run (its status copy included)
    double *win = nullptr, *win2 = nullptr, *pinv = nullptr, *basis = nullptr;
    tts::DeviceBuf<int> NS;  // analysis: samples per sentence; linear -> mel: frames per sentence
    int* band = nullptr;  // [num_mels][2] nonzero bin range of each mel basis row
    int band_lo = 0, band_hi = 0;  // their union
    double2* tw = nullptr;
    double2* wt = nullptr;  // gl_iter_wave_kernel pass-2 twiddles [16][4]
    double2* winc = nullptr;  // gl_iter_wave_kernel window rotation bases [4][64]
    float* wssp = nullptr;    // gl_ola_kernel periodic window sum-square [hop]
    double wrot = 0.0;
    bool wave = true;       // batched iterations on gl_iter_wave_kernel (TTS_GL_WAVE=0: gl_iter_kernel)
    // workspace
    tts::DeviceBuf<tts::spec_t> S;
    tts::DeviceBuf<tts::frame_t> frames;  // ping-pong slots
    tts::DeviceBuf<float> y;
    tts::DeviceBuf<int> F;
    std::map<tts::GraphKey, hipGraphExec_t> graphs;
    float last_ms = 0.f;
    int last_launches = 0;
    bool last_fused = false;
    bool last_persistent = false;
    int last_path = TTS_GL_PATH_UNFUSED;
    tts::DeviceBuf<unsigned> flags;  // persistent loop: the workgroups' XCD table
    tts::DeviceBuf<tts::gran_t> pgr;  // persistent loop: two granule slots
    std::vector<signed char> gather_fit;  // by frame count: the persistent loop's contributor relation is
                                          // symmetric and its gather layout holds (-1: unknown)
    int* pstatus = nullptr;     // [dev] status of the persistent loop
    int* host_status = nullptr; // pinned coherent: [0] status of the last persistent loop, [1] its sequence
    int seq = 0;                // pipeline mode: the sequence the last persistent run's overlap-add sets
    hipStream_t seq_stream = nullptr;
    unsigned salt = 0;
    long long tmo = 0;
    bool have_last = false;
    tts::IterArgs last_iter{};
    bool pipeline = false;        // tts_synth_run: caller's stream, completion collected later
    bool pending = false;         // a pipeline run whose timing / status is not collected yet
    bool last_timed = true;       // the last run recorded its events (not in pipeline mode)
    tts::FinArgs last_fin{};
    size_t last_fstride = 0;
    // numpy-stream initial phases (tts_gl_set_phase_state, phase_mt.hip): the MT19937 state on the
    // device, the phases it drew for the current run, the stream and event of its last draw
    bool mt_armed = false;
    unsigned* mt_state = nullptr;  // [625] key + position
    tts::DeviceBuf<double> mt_phase;  // [B][1025][Fmax]
    tts::DeviceBuf<int> mt_F;      // tts_gl_draw_phases: the frame counts on the device
    hipStream_t mt_stream = nullptr;
    hipEvent_t ev_mt = nullptr;
    tts::MtWork mt_work;           // the draws' device workspace (phase_mt.hip)
    // tts_gl_save_pcm16: the peak word and the output offsets ([dev], host copy kept for the upload)
    unsigned long long* pcm_peak = nullptr;
    tts::DeviceBuf<int64_t> pcm_start;
    std::vector<int64_t> pcm_start_h;
    // tts_gl_trim_silence / tts_gl_find_endpoint: one value per frame / candidate window, then the
    // counts and the integer results ([dev], bytes, grown on demand; both calls return with it idle)
    tts::DeviceBuf<char> sil;
    // tts_gl_take_segments: start / len per sentence ([dev], host copy kept for the upload)
    tts::DeviceBuf<int> seg;
    std::vector<int32_t> seg_h;
    // tts_gl_set_resample_filter / tts_gl_resample: the half window ([dev]), the time registers by
    // (orig_sr, target_sr), the sentences of the current call ([dev], host copy kept for the upload)
    tts::DeviceBuf<double> rs_win;
    int rs_nwin = 0, rs_table = 0;
    std::map<std::pair<int, int>, tts::RsRegister> rs_reg;
    tts::DeviceBuf<tts::RsSent> rs_sent;
    std::vector<tts::RsSent> rs_sent_h;
};

namespace tts {
// phase_mt.hip: numpy-stream phases for a run of B sentences (F_dev on the device, read on s) into
// `out` ([B][1025][Fmax]), continuing the handle's MT19937 state
tts_status mt_draw(tts_gl* g, const int* F_dev, int B, int Fmax, double* out, hipStream_t s);
}  // namespace tts
