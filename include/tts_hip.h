/*
 * tts_hip.h — C-ABI of libtts_hip.so, the MI355X (gfx950) synthesis path of the
 * prototypefund/your-voice-TTS drop-in.
 *
 * The reference has no FFI for this path: it is pure Python on stock PyTorch ops and librosa
 * (SURVEY.md §0.1).  Each entry point below replaces one reference call site; the host package
 * (your-voice-tts_amd/) binds them with ctypes and keeps the reference's Python signatures.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Pointers marked [dev] are device (HBM) pointers, [host]
 *     are host pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Caller owns all input/output buffers; the library owns weights, workspace and graphs.
 *   - Every call returns a tts_status; tts_last_error() gives the message of the last failure
 *     on the calling thread.  No exceptions cross the ABI.
 *   - A handle is not reentrant: one thread/stream per handle at a time (the reference decoder
 *     keeps per-call state on the module and is not reentrant either, layers/tacotron2.py:161-177).
 *   - Model arithmetic is fp32 (as the reference's torch modules); Griffin-Lim magnitudes, FFTs
 *     and the inverse pre-emphasis are fp64 (scipy.fftpack / scipy.signal.lfilter precision).
 */
#ifndef TTS_HIP_H
#define TTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int tts_status;
#define TTS_OK 0
#define TTS_ERR_INVALID 1     /* bad argument / shape / missing weight            */
#define TTS_ERR_HIP 2         /* HIP runtime error (message in tts_last_error)    */
#define TTS_ERR_UNSUPPORTED 3 /* configuration the path does not implement        */
#define TTS_ERR_NOMEM 4

typedef struct tts_encoder tts_encoder;
typedef struct tts_decoder tts_decoder;
typedef struct tts_postnet tts_postnet;
typedef struct tts_gl tts_gl;
typedef struct tts_tacotron tts_tacotron;

/* One weight tensor in the reference's own state_dict layout (fp32, contiguous, [dev]). */
typedef struct tts_tensor {
    const char* key;   /* reference state_dict key, e.g. "decoder.attention_rnn.weight_ih" */
    const float* data; /* [dev] fp32                                                        */
    int64_t numel;
} tts_tensor;

/* Replaces the embedding lookup + Encoder.inference of Tacotron2.inference (models/tacotron2.py:
 * 63-64, layers/tacotron2.py:48-83): 3 x (Conv1d k=5 + BatchNorm + ReLU) and the bidirectional
 * LSTM.  `tensors` must hold embedding.weight and every encoder.* key. */
tts_status tts_encoder_create(const tts_tensor* tensors, int n_tensors, int max_batch, int max_len,
                              void* stream, tts_encoder** out);
void tts_encoder_destroy(tts_encoder* e);
/*   ids  [dev]  int32 [B][Lmax] character ids (entries past lens[b] ignored)
 *   lens [host] int32 [B], 1 <= lens[b] <= Lmax
 *   out  [dev]  fp32 [B][Lmax][512]; each sentence is encoded at its own length, rows past
 *                lens[b] are zero. */
tts_status tts_encoder_run(tts_encoder* e, const int32_t* ids, const int32_t* lens, int B, int Lmax,
                           float* out, void* stream);
/* Same with the BiLSTM state carried (Encoder.inference_truncated, layers/tacotron2.py:85-93):
 *   state_in  [dev] fp32 [4][B][256] = (h_fwd, h_bwd, c_fwd, c_bwd) initial state, or NULL (zeros)
 *   state_out [dev] fp32 [4][B][256] final state (h_n, c_n per direction), or NULL.
 * Which BiLSTM serves which arguments (reported by tts_encoder_last_path); out and state_out are
 * the same on every path within fp32 reduction order:
 *   B == 1, lens[0] == Lmax, state_in given or NULL ..... resident batch-1 launch (1)
 *   B == 1, lens[0] <  Lmax ............................. per-step launches (0)
 *   B >= 2, state_in == NULL, state_out given or NULL ... batched resident launch (2), which
 *                                                         stores h_n / c_n of every sentence itself
 *   B >= 2, state_in given .............................. per-step launches (0)
 * A handle created under TTS_RESIDENT=0, or on a device where a resident grid cannot be placed,
 * serves everything with the per-step launches; a resident launch whose hand-off wait times out is
 * rerun per-step from the caller's initial state within the same call. */
tts_status tts_encoder_run_state(tts_encoder* e, const int32_t* ids, const int32_t* lens, int B, int Lmax,
                                 const float* state_in, float* state_out, float* out, void* stream);

/* Tacotron2._add_speaker_embedding (models/tacotron2.py:65, 91-100) on an encoder output:
 * enc[b][t] += speaker_embedding.weight[speaker_ids[b]] for t < lens[b] (rows past stay zero).
 * The handle must have been created with speaker_embedding.weight among its tensors.
 *   enc [dev] fp32 [B][Lmax][512]; lens, speaker_ids [host] int32 [B] (B <= 64) */
tts_status tts_encoder_add_speakers(tts_encoder* e, float* enc, const int32_t* lens, const int32_t* speaker_ids, int B,
                                    int Lmax, void* stream);

/* The last run's BiLSTM path: 1 the resident batch-1 launch, 2 the batched resident launch
 * (2 <= B <= 64), 0 the per-step launches (see tts_encoder_run_state). */
tts_status tts_encoder_last_path(tts_encoder* e, int* resident);
/* Resident batch-1 launches of this handle that were rerun with the per-step launches: because the
 * runtime placed too few workgroups on an XCD (placement_failures), or because a hand-off wait
 * timed out beside another stream's work (timeouts). */
tts_status tts_encoder_counters(tts_encoder* e, int* placement_failures, int* timeouts);
/* The rule a handle applies to the status word (salt << 8 | code) of its resident batch-1 launch
 * `salt`; host arithmetic only, no device.  *outcome: TTS_ENC_RUN_OK (and *fails_in_row = 0),
 * TTS_ENC_RUN_PLACEMENT (++*fails_in_row; *resident = 0 once that reaches 3 sentences in a row, the
 * decoder's rule) or TTS_ENC_RUN_TIMEOUT (both unchanged).  Either failure reruns that sentence
 * per-step. */
#define TTS_ENC_RUN_OK 0
#define TTS_ENC_RUN_PLACEMENT 1
#define TTS_ENC_RUN_TIMEOUT 2
tts_status tts_encoder_status_rule(int status_word, unsigned salt, int* fails_in_row, int* resident, int* outcome);

/* Decoder flags: the arguments of layers/tacotron2.py:98-100 (Decoder.__init__) that change
 * inference numerics, as mapped from the JSON config by utils/generic_utils.py:275-288. */
typedef struct tts_decoder_config {
    int r;                 /* frames per step (config "r")                                 */
    int attn_norm;         /* 0 = softmax, 1 = sigmoid (common_layers.py:239-245)          */
    int forward_attn;      /* use_forward_attn                                             */
    int trans_agent;       /* transition_agent                                             */
    int forward_attn_mask; /* forward_attn_mask (synthesize.py:86 forces 1)                */
    int location_attn;     /* location_attn                                                */
    int windowing;         /* windowing (attn_win), eval-only window (common_layers.py:184) */
    int max_batch;         /* workspace capacity: sentences per call (<= 64)              */
    int max_len;           /* workspace capacity: encoder length L (<= 1024)              */
    int max_steps;         /* workspace capacity: decoder steps (max_decoder_steps)        */
} tts_decoder_config;

/* Replaces the construction + load_state_dict of layers/tacotron2.py:97-150 (Decoder).
 * `tensors` must hold every decoder.* key of the reference state_dict for this config; they
 * are repacked into the library's MFMA-fragment layout (the caller may free them after).
 * prenet_type "bn" (common_layers.py:28-70) is selected by the presence of the
 * decoder.prenet.layers.{0,1}.bn.* keys (eval-mode BatchNorm1d, folded into the prenet at create;
 * tts_tacotron_create does the same for its decoder prenet). */
tts_status tts_decoder_create(const tts_decoder_config* cfg, const tts_tensor* tensors, int n_tensors,
                              void* stream, tts_decoder** out);
void tts_decoder_destroy(tts_decoder* d);

/* Replaces Decoder.inference (layers/tacotron2.py:249-285) for a padded batch of sentences,
 * with per-sentence semantics identical to the reference run alone at batch 1:
 *   enc      [dev]  fp32 [B][Lmax][512] encoder outputs (rows >= lens[b] ignored)
 *   lens     [host] int32 [B] encoder lengths L_b (2 <= L_b <= Lmax <= cfg.max_len)
 *   max_steps        the reference's max_decoder_steps (<= cfg.max_steps)
 *   mel      [dev]  fp32 [B][steps_cap*r][80]  mel frames (decoder_output, time-major)
 *   stop     [dev]  fp32 [B][steps_cap]        sigmoid(stop token)
 *   align    [dev]  fp32 [B][steps_cap][Lmax]  attention weights per step (may be NULL)
 *   n_steps  [host] int32 [B] out: decoder steps taken by each sentence
 * steps_cap must be >= max_steps + 20 (the reference can run up to 20 steps past the cap once
 * every stop flag is set, layers/tacotron2.py:271-277).  Entries past n_steps[b] are zero up
 * to the batch's longest run and left untouched beyond it.  Synchronises `stream` once per
 * chunk of steps to read the stop flags. */
tts_status tts_decoder_run(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax,
                           int max_steps, int steps_cap, float* mel, float* stop, float* align,
                           int32_t* n_steps, void* stream);

/* Continuous mode: replaces Decoder.inference_truncated (layers/tacotron2.py:287-328).  Same
 * arguments as tts_decoder_run, batch 1 only; the attention-LSTM / decoder-LSTM states, the
 * context and the memory (last mel frame) carry over from the previous batch-1 run on this handle,
 * the attention and stop-rule state restart. */
tts_status tts_decoder_run_continue(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax,
                                    int max_steps, int steps_cap, float* mel, float* stop, float* align,
                                    int32_t* n_steps, void* stream);

/* Teacher forcing: replaces Decoder.forward(inputs, memories, mask) (layers/tacotron2.py:227-247)
 * in eval mode.  Step t decodes from the go frame (t = 0) or teacher row t-1 (80*r values: frames
 * (t-1)r .. tr-1), with no stop rule: exactly `steps` steps for every sentence, each sentence at its
 * own encoder length (padding positions are never attended, as the reference's mask would do).
 *   memories [dev] fp32 [B][mem_ldb] teacher frames, row t at t * 80 * r
 *   mel   [dev] fp32 [B][steps][80*r]; stop [dev] fp32 [B][steps] stopnet LOGITS (no sigmoid, as
 *         Decoder.forward returns them); align [dev] fp32 [B][steps][Lmax] or null. */
tts_status tts_decoder_run_teacher(tts_decoder* d, const float* enc, const int32_t* lens, int B, int Lmax,
                                   const float* memories, int64_t mem_ldb, int steps, float* mel, float* stop,
                                   float* align, void* stream);

/* Per-step timing of the last tts_decoder_run (ms of GPU time of the step loop, steps run). */
tts_status tts_decoder_last_timing(tts_decoder* d, float* loop_ms, int* steps_run);

/* Which implementation ran the last tts_decoder_run / _continue (no reference counterpart):
 * *resident = 1 for the resident single-launch batch-1 decoder (every step weight held on chip
 * by 256 workgroups, hand-offs in device memory), 2 for the resident batch decoder (the same for
 * up to 4 sentences per launch, both LSTMs' rows in registers; consecutive launches for larger
 * batches), 0 for the per-step multi-launch hipGraph path.  The batch-1 path serves L <= 256 under
 * every Tacotron2 attention configuration, the batch path 2 <= B <= 8 with every L_b <= 256 under
 * the same configurations (location features, windowing and the transition agent in its general
 * attention form); both need >= 256 compute units.
 * TTS_RESIDENT=0 / TTS_RESIDENT_BATCH=0 in the environment at tts_decoder_create disable them;
 * TTS_RB_GENERAL=0 keeps only the location / windowing / transition-agent configurations off the
 * batch path (batch-1 resident calls or multi-launch, as before the general form existed). */
tts_status tts_decoder_last_path(tts_decoder* d, int* resident);
/* The requests the resident decoder serves on this handle now: batches of at most *max_batch
 * sentences of encoder length <= *max_len (both 0: the handle runs multi-launch only, e.g. after
 * repeated placement failures).  Callers that split a request (Synthesizer.tts's dispatch) gate on it. */
tts_status tts_decoder_resident_limits(tts_decoder* d, int* max_batch, int* max_len);

/* Measurement only: re-runs the last resident batch-1 sentence with phase timers and returns the
 * mean microseconds per decoder step of each phase, us[0..15] on compute unit 0 and us[16..31] on
 * the attention compute unit (n >= 32): 0 attention-LSTM early part + wait pre1, 1 prenet-2 row
 * (0-1 on the prenet compute units), 2 wait prenet-2, 3 attention-LSTM prenet part, 4 cell + gather
 * h_att, 5 query row + decoder-LSTM early part, 6 wait query, 7 energies + max(alpha), 8 weights,
 * context, publish, 9 next-step prefetch (6-9 attention CU only), 10 wait context, 11 decoder-LSTM
 * context part, 12 cell + gather h_dec, 13 fused mel / prenet-1 / stop rows (wave 2); 14 and 15 split
 * 7 and 8 (candidate energies up to their barrier; window weights + context before publishing). */
#define TTS_RESIDENT_PHASES 16
tts_status tts_decoder_resident_phases(tts_decoder* d, float* us, int n);
// Measurement only: re-runs the last resident sentence with per-CU event stamps (no phase marks) and
// returns n >= 256*64*12 wall-clock ticks [CU][step < 64][event]: P1, B1, h_att published, B3, B4,
// h_dec published, B6, pre1 row published, query row published, and on the attention CUs A1 (query
// gathered), A2 (candidate energies), context published (0 = not reached).
tts_status tts_decoder_resident_trace(tts_decoder* d, long long* ticks, int64_t n);

/* Measurement only (no reference counterpart): re-runs up to `reps` steps of the last
 * tts_decoder_run's batch eagerly, with a HIP event before/after every kernel on the stream it
 * is launched on, and returns the mean duration (ms) of each step kernel, in launch order:
 * prenet2, attention-LSTM, query, attention, decoder-LSTM, fused mel/prenet1/stop.
 * Leaves the decoder state mid-sentence (the next tts_decoder_run re-initialises it). */
#define TTS_DECODER_STEP_KERNELS 6
tts_status tts_decoder_profile(tts_decoder* d, int reps, float* kernel_ms, int n_kernels);

/* Replaces Postnet (layers/tacotron2.py:30-45) + the residual add of models/tacotron2.py:69-70:
 * out = mel + postnet(mel), per sentence at its own length (zero padding past T_b).
 * `tensors` must hold the postnet.* keys. */
tts_status tts_postnet_create(const tts_tensor* tensors, int n_tensors, int n_mel, void* stream,
                              tts_postnet** out);
void tts_postnet_destroy(tts_postnet* p);
/*   mel [dev] fp32 [B][Tmax][n_mel] time-major; T [host] int32 [B]; out [dev] same shape.
 * Rows t >= T[b] of mel are never read and may hold anything (NaN included); rows t >= T[b] of
 * out are never written (they keep what the caller put there).  T[b] = 0 is legal: that sentence
 * is neither read nor written.  Tmax may exceed the longest T[b]. */
tts_status tts_postnet_run(tts_postnet* p, const float* mel, const int32_t* T, int B, int Tmax,
                           float* out, void* stream);
/* Which convolution kernel served each of the five layers of the last tts_postnet_run (no
 * reference counterpart): kinds[0..4], n >= 5, -1 before the first run.  0 small-batch kernel
 * with channel-major weights, 1 small-batch tap-major with 32 output channels per workgroup,
 * 2 the same with 16, 3 tiled with 16-frame tiles, 4 split-K plus a reduce launch, 5 split-K
 * reducing in the same launch (TTS_CONV_FUSED_REDUCE=1), 6 variable-length 64-frame tiles,
 * 7 tiled 32-frame, 8 tiled 64-frame.  The host chooses by sum T[b], B * ceil(max T[b] / 16),
 * the layer's channels and TTS_CONV_VL. */
tts_status tts_postnet_last_path(tts_postnet* p, int* kinds, int n);

/* Audio parameters of AudioProcessor (utils/audio.py:12-54, 114-119). */
typedef struct tts_audio_config {
    int n_fft;          /* (num_freq-1)*2, must be 2048 */
    int hop_length;     /* frame_shift_ms * sample_rate / 1000 */
    int win_length;     /* frame_length_ms * sample_rate / 1000, <= n_fft */
    int num_mels;
    float min_level_db, ref_level_db, power, max_norm;
    double preemphasis; /* lfilter coefficient, kept in double as the reference's Python float */
    int signal_norm, symmetric_norm, clip_norm;
} tts_audio_config;

#define TTS_GL_FROM_MEL 0     /* AudioProcessor.inv_mel_spectrogram (utils/audio.py:164-172) */
#define TTS_GL_FROM_LINEAR 1  /* AudioProcessor.inv_spectrogram     (utils/audio.py:154-162) */

/* inv_mel_basis: [host] fp64 [n_fft/2+1][num_mels] = pinv(mel basis) (utils/audio.py:64-66);
 * may be NULL when only the linear path is used.  Magnitudes, FFTs and the phase are float64,
 * the STFT is rounded to complex64 and the signal kept float32, as librosa 0.6.2 does. */
tts_status tts_gl_create(const tts_audio_config* cfg, const double* inv_mel_basis, void* stream, tts_gl** out);
void tts_gl_destroy(tts_gl* g);

/* Batched Griffin-Lim vocoder: replaces inv_mel_spectrogram / inv_spectrogram, i.e.
 * denormalise -> dB->amp -> [pinv mel->linear] -> ^power -> _griffin_lim (utils/audio.py:182-201,
 * librosa 0.6.2 stft/istft) -> inverse pre-emphasis (lfilter, utils/audio.py:133-136).
 *   spec    [dev]  fp32 [B][Fmax][n_in] frame-major (n_in = num_mels or n_fft/2+1 by mode)
 *   F       [host] int32 [B] frames per sentence (>= 2)
 *   phase_u [dev]  fp64 [B][n_fft/2+1][Fmax] initial phases as U[0,1) draws (the reference's
 *                  np.random.rand(*S.shape)), or NULL: drawn on device from `seed`
 *   wav     [dev]  fp64 [B][hop*(Fmax-1)]: sentence b fills its first hop*(F_b-1) samples */
tts_status tts_gl_run(tts_gl* g, int mode, const float* spec, const int32_t* F, int B, int Fmax,
                      const double* phase_u, uint64_t seed, int iters, double* wav, void* stream);

/* numpy-stream initial phases.  The reference draws each sentence's initial Griffin-Lim phases
 * with np.random.rand(*S.shape) from numpy's global legacy generator (utils/audio.py:183), sentence
 * after sentence (server/synthesizer.py:145-158).  tts_gl_set_phase_state takes that generator's
 * state (np.random.get_state(): MT19937 key[624] and position 0..624) and arms the handle: every
 * following tts_gl_run with phase_u == NULL (and the runs of a tts_synth on this handle) draws its
 * phases from it ON THE DEVICE, one [n_fft/2+1][F_b] draw per sentence in batch order, bitwise the
 * values np.random.rand returns, and advances the state; key == NULL disarms (device-seeded phases
 * again).  tts_gl_get_phase_state waits for the last draw and returns the state numpy would hold
 * after the same draws (np.random.set_state it back).  tts_gl_draw_phases draws into phase_u [dev]
 * fp64 [B][n_fft/2+1][Fmax] directly (F [host] int32 [B], 0 <= F[b] <= Fmax, B <= 1024). */
tts_status tts_gl_set_phase_state(tts_gl* g, const uint32_t* key, int pos);
tts_status tts_gl_get_phase_state(tts_gl* g, uint32_t* key, int* pos);
tts_status tts_gl_draw_phases(tts_gl* g, const int32_t* F, int B, int Fmax, double* phase_u, void* stream);

/* Synthesizer.tts's join + AudioProcessor.save_wav's int16 conversion (server/synthesizer.py:157-161,
 * utils/audio.py:56-58), on the device: sentence b's first n[b] samples, each sentence followed by
 * `gap` zeros (10000 in the reference), scaled by 32767 / max(0.01, peak) and truncated to int16, with
 * numpy's float64 arithmetic (the bytes of the reference's wav).  peak < 0: max |y| over the request;
 * peak >= 0: that value (a sharded request's all-ranks maximum).
 *   wav [dev] fp64 [B][pitch]; n [host] int64 [B]; out [dev] int16 [sum(n[b] + gap)] */
tts_status tts_gl_save_pcm16(tts_gl* g, const double* wav, int64_t pitch, const int64_t* n, int B, int gap,
                             double peak, int16_t* out, void* stream);

/* AudioProcessor.trim_silence (utils/audio.py:212-217) for a ragged batch on the device: per sentence the
 * signal is wav[b][margin : N[b] - margin] (n_b samples), and librosa 0.6.2 effects.trim runs on it: reflect
 * padding by frame_length / 2 (index arithmetic, no padded copy), 1 + n_b / hop_length frames centred on
 * sample t * hop_length, float64 mean square per frame (one fixed summation order: bitwise run to run),
 * 10 log10(max(1e-10, .)) against the loudest frame, the frames above -top_db kept.  Relative to the
 * margin-stripped signal, as the reference's slice: start = first_kept * hop_length, end = min(n_b,
 * (last_kept + 1) * hop_length); both 0 when no frame is kept.  No sample at or beyond N[b] is read.
 * INVALID before any launch: a null pointer, B <= 0, N[b] > pitch, N[b] < 2 * margin, a non-positive hop, a
 * frame length that is not positive and even, and a sentence with n_b < frame_length / 2 + 1 (the padding would need a second reflection;
 * numpy's pad raises there too): the error text names the sentence.  Waits for the stream before it returns.
 *   wav [dev] fp64 [B][pitch]; N [host] int32 [B]; start_out, end_out [host] int32 [B] */
tts_status tts_gl_trim_silence(tts_gl* g, const double* wav, int64_t pitch, const int32_t* N, int B, int margin,
                               int frame_length, int hop_length, double top_db, int32_t* start_out,
                               int32_t* end_out, void* stream);

/* AudioProcessor.find_endpoint (utils/audio.py:203-210, the cut of utils/synthesis.py:59-60, 122-123) for a
 * ragged batch on the device: the candidates are x = k * hop_length, k >= 1, x < N[b] - window_length
 * (strict, Python's range); the first whose maximum over wav[b][x : x + window_length] is < threshold gives
 * x + hop_length, and N[b] when there is none.  As in the reference the maximum is of the signed samples
 * (not of |y|) and the comparison is strict; window_length need not be a multiple of hop_length.  A maximum
 * rounds nothing: the integers are numpy's.  `threshold` is the caller's 10^(threshold_db * 0.05).
 * INVALID before any launch: a null pointer, B <= 0, N[b] outside [0, pitch], a non-positive hop or window.
 * Waits for the stream before it returns.
 *   wav [dev] fp64 [B][pitch]; N [host] int32 [B]; end_out [host] int32 [B] */
tts_status tts_gl_find_endpoint(tts_gl* g, const double* wav, int64_t pitch, const int32_t* N, int B,
                                int window_length, int hop_length, double threshold, int32_t* end_out,
                                void* stream);

/* The slices the two calls above describe (wav[start:end] of utils/audio.py:217, wav[:end] of
 * utils/synthesis.py:60), gathered for the analysis entry points: dst[b][0 : len[b]] = src[b][start[b] :
 * start[b] + len[b]], zeros from len[b] to dst_pitch.  Enqueued on `stream`; does not wait.
 * INVALID before any launch: a null pointer, B <= 0, a negative start or len, start[b] + len[b] > src_pitch,
 * len[b] > dst_pitch, dst_pitch < 1.
 *   src [dev] fp64 [B][src_pitch]; start, len [host] int32 [B]; dst [dev] fp64 [B][dst_pitch] */
tts_status tts_gl_take_segments(tts_gl* g, const double* src, int64_t src_pitch, const int32_t* start,
                                const int32_t* len, int B, double* dst, int64_t dst_pitch, void* stream);

/* The interpolation filter of the resampler below (utils/audio.py:239: librosa.load resamples with resampy's
 * "kaiser_best"): the right half of a windowed sinc, num_table entries per zero crossing, as
 * resampy.filters.sinc_window returns it (kaiser_best: n_win 32 769, num_table 512).  Copied to the device;
 * replaces the handle's previous filter.  INVALID: a null pointer, a non-positive n_win or num_table.
 *   half_win [host] fp64 [n_win] */
tts_status tts_gl_set_resample_filter(tts_gl* g, const double* half_win, int n_win, int num_table);

/* librosa.load's resampler (utils/audio.py:239; librosa 0.6.2 resample with fix=True, resampy 0.2.x resample_f)
 * for a ragged batch on the device, one launch: sentence b goes from orig_sr[b] to target_sr.  With
 * ratio = target_sr / orig_sr[b] it has n_res = int(N[b] * ratio) outputs and n_fix = ceil(N[b] * ratio)
 * samples (fix_length; those at and beyond n_res are zero).  Every source value is rounded to float32 on load
 * (librosa hands resampy float32), the accumulator of an output is float32, every tap is one fp64 multiply,
 * one fp64 add and one rounding to float32 in resampy's order, and the time register is resampy's serial
 * float64 sum (built on the host once per rate pair, cached on the handle): the result equals resampy's bit
 * for bit, each value a float32.  A sentence with orig_sr[b] == target_sr passes through.  No sample at or
 * beyond N[b] is read; dst is zero from n_res to dst_pitch, so it feeds tts_gl_trim_silence,
 * tts_gl_take_segments and tts_gl_analyze as it is.  n_out receives n_fix.
 * INVALID before any launch: a null pointer, B <= 0, a non-positive rate, N[b] outside [1, src_pitch],
 * n_res < 1, n_fix > dst_pitch, no filter set, step = int(min(1, ratio) * num_table) < 1, wings longer than
 * the 16 384 inputs a workgroup stages (kaiser_best: a ratio below 5 / 512): the error text names the
 * sentence.  Waits for the stream before it returns.
 *   src [dev] fp64 [B][src_pitch]; N, orig_sr [host] int32 [B]; dst [dev] fp64 [B][dst_pitch];
 *   n_out [host] int32 [B] */
tts_status tts_gl_resample(tts_gl* g, const double* src, int64_t src_pitch, const int32_t* N,
                           const int32_t* orig_sr, int target_sr, int B, double* dst, int64_t dst_pitch,
                           int32_t* n_out, void* stream);

/* Mel analysis for GST style wavs: AudioProcessor.melspectrogram (utils/audio.py:146-152) as used by
 * compute_style_mel (utils/synthesis.py:28-35): pre-emphasis FIR, librosa 0.6.2 stft (float64 FFT,
 * complex64 result), |D|, mel projection (float64), amp->dB, _normalize.
 *   mel_basis [host] fp64 [num_mels][n_fft/2+1] (librosa filters.mel), set once per handle (each row's
 *   nonzero bin range is found here and kept on the device for tts_gl_linear_to_mel)
 *   wav [dev] fp64 [B][Nmax]; N [host] int32 [B] (>= 2); mel [dev] fp32 [B][Fmax][num_mels]
 *   (frame-major; sentence b has 1 + N[b]/hop frames, the rest zero). */
tts_status tts_gl_set_mel_basis(tts_gl* g, const double* mel_basis);
tts_status tts_gl_melspectrogram(tts_gl* g, const double* wav, const int32_t* N, int B, int64_t Nmax, float* mel,
                                 int Fmax, void* stream);

/* The analysis half of AudioProcessor from one STFT: spectrogram (utils/audio.py:138-144), melspectrogram
 * (:146-152), or both as collate_fn computes them for every wav (datasets/TTSDataset.py:191-192).  One
 * launch and one FFT per frame whichever outputs are asked for; at least one must be non-NULL, and `mel`
 * needs tts_gl_set_mel_basis first.  Bin k of the linear output is 20 log10(max(min_level, |D_k|)) -
 * ref_level_db through _normalize (all four flags, max_norm), |D_k| the float32 magnitude of the complex64
 * STFT value; the mel output is bitwise tts_gl_melspectrogram's.
 *   wav [dev] fp64 [B][Nmax]; N [host] int32 [B] (2 <= N[b] <= Nmax; Fmax >= 1 + N[b]/hop)
 *   linear [dev] fp32 [B][Fmax][n_fft/2+1] or NULL; mel [dev] fp32 [B][Fmax][num_mels] or NULL
 *   (frame-major, the layout tts_gl_run(TTS_GL_FROM_LINEAR) reads; rows at and beyond 1 + N[b]/hop zero). */
tts_status tts_gl_analyze(tts_gl* g, const double* wav, const int32_t* N, int B, int64_t Nmax, float* linear,
                          float* mel, int Fmax, void* stream);

/* AudioProcessor.out_linear_to_mel (utils/audio.py:174-180): a model's normalised linear spectrogram to the
 * normalised mel an external vocoder reads, per frame _denormalize -> + ref_level_db -> 10^(x*0.05)
 * (float32) -> mel_basis . S (float64, summed over each basis row's nonzero bins only) -> _amp_to_db -
 * ref_level_db -> _normalize.  Needs tts_gl_set_mel_basis first.
 *   linear [dev] fp32 [B][Fmax][n_fft/2+1]; F [host] int32 [B] (1 <= F[b] <= Fmax)
 *   mel [dev] fp32 [B][Fmax][num_mels] (rows at and beyond F[b] zero). */
tts_status tts_gl_linear_to_mel(tts_gl* g, const float* linear, const int32_t* F, int B, int Fmax, float* mel,
                                void* stream);

/* Time of the last tts_gl_run's iteration loop (ms, GPU) and kernel launches in it. */
tts_status tts_gl_last_timing(tts_gl* g, float* loop_ms, int* launches);

/* Iteration loop the last tts_gl_run took: TTS_GL_PATH_UNFUSED (overlap-add launch + per-frame
 * STFT/iSTFT launch per iteration), TTS_GL_PATH_FUSED (one launch per iteration), or
 * TTS_GL_PATH_PERSISTENT (every iteration in one co-resident launch, up to 512 frames in all: one
 * workgroup per frame, one per compute unit up to 256 workgroups and two per compute unit above;
 * when the grid cannot be co-resident the run falls back to the fused loop, bitwise the same
 * waveform). */
#define TTS_GL_PATH_UNFUSED 0
#define TTS_GL_PATH_FUSED 1
#define TTS_GL_PATH_PERSISTENT 2
tts_status tts_gl_last_path(tts_gl* g, int* path);

/* Measurement only: re-runs `reps` GL iterations of the last tts_gl_run's batch eagerly with
 * HIP events around each kernel on its stream; returns mean ms of [per-frame STFT/iSTFT kernel,
 * overlap-add kernel] (one iteration launches both).  Clobbers the internal frame and signal
 * buffers (not the caller's outputs). */
#define TTS_GL_KERNELS 2
tts_status tts_gl_profile(tts_gl* g, int reps, float* kernel_ms, int n_kernels);

/* ---------------------------------------------------------------- whole-sentence synthesis
 * Replaces utils/synthesis.py:synthesis for Tacotron2 (model.inference, :50-57,
 * then ap.inv_mel_spectrogram of the postnet output, :69-77) in ONE call over the handles above:
 * tts_encoder_run -> tts_decoder_run -> tts_postnet_run -> tts_gl_run (mel mode, device phases
 * from `seed`), bitwise the same as calling them one by one, without the host round trips in
 * between.  The handles stay owned by the caller and must outlive the tts_synth. */
typedef struct tts_synth tts_synth;
tts_status tts_synth_create(tts_encoder* e, tts_decoder* d, tts_postnet* p, tts_gl* g, int r, int n_mel, int hop,
                            tts_synth** out);
void tts_synth_destroy(tts_synth* s);
/*   ids    [host] int32 [B][Lmax]; lens [host] int32 [B], 2 <= lens[b] <= Lmax
 *   wav    [dev]  fp64 [B][hop*(Fmax-1)] out, Fmax = max frames[b] (wav_cap = elements available)
 *   frames [host] int32 [B] out: mel frames of each sentence (decoder steps * r); sentence b's
 *          waveform is the first hop*(frames[b]-1) samples of its row, the rest zero. */
tts_status tts_synth_run(tts_synth* s, const int32_t* ids, const int32_t* lens, int B, int Lmax, int max_steps,
                         int gl_iters, uint64_t seed, double* wav, int64_t wav_cap, int32_t* frames, void* stream);
/* tts_synth_run for a multi-speaker Tacotron2 (utils/synthesis.py:synthesis with speaker_id):
 * the speaker embedding is added to the encoder output (tts_encoder_add_speakers) before the decoder.
 *   speaker_ids [host] int32 [B] */
tts_status tts_synth_run_speakers(tts_synth* s, const int32_t* ids, const int32_t* lens, const int32_t* speaker_ids,
                                  int B, int Lmax, int max_steps, int gl_iters, uint64_t seed, double* wav,
                                  int64_t wav_cap, int32_t* frames, void* stream);
/* tts_synth_run returns once Griffin-Lim is enqueued; its completion status (a persistent loop's
 * hand-off timeout) is otherwise collected by the next run.  This waits for the last run and
 * returns that status.  A failed run's waveform is NaN, never a plausible-looking signal. */
tts_status tts_synth_sync(tts_synth* s);
/* *last_front: the last run's encoder stage ran on the handle's own stream, beside the work the
 * caller's stream still had in flight (batch 1 only; TTS_SYNTH_FRONT=0 turns it off);
 * *in_flight (or NULL: not asked): a stream this handle's runs work on still has work queued
 * (stream queries, no wait). */
tts_status tts_synth_state(tts_synth* s, int* last_front, int* in_flight);

/* ---------------------------------------------------------------- Tacotron / TacotronGST
 * SURVEY config 5 (config_tacotron_gst.json) and config_tacotron.json: the r-frames-per-step
 * Tacotron family, models/tacotron.py / models/tacotrongst.py. */
/* Longest decoder memory queue, in frames: the prenet reads 80 * memory_size values
 * (layers/tacotron.py:279-287), at most 1280. */
#define TTS_TACOTRON_MEMORY_SIZE_MAX 16
typedef struct tts_tacotron_config {
    int r;                 /* frames per step                                                  */
    int memory_size;       /* decoder memory queue in frames (<= 0 means r): r <= memory_size  */
                           /* <= TTS_TACOTRON_MEMORY_SIZE_MAX; a shorter queue is INVALID (the */
                           /* reference cannot run it either)                                  */
    int attn_norm;         /* 0 = softmax, 1 = sigmoid                                         */
    int forward_attn, trans_agent, forward_attn_mask, location_attn, windowing;
    int gst;               /* 1: TacotronGST (gst.* weights present), 0: Tacotron              */
    int num_speakers;      /* > 1: speaker_embedding.weight present                            */
    int max_batch;         /* workspace capacity: sentences per call (<= 64)                   */
    int max_len;           /* workspace capacity: encoder length (<= 1024, 512 with location)  */
    int max_steps;         /* workspace capacity: decoder steps (max_decoder_steps)            */
} tts_tacotron_config;

/* Replaces construction + load_state_dict of TacotronGST / Tacotron (models/tacotrongst.py:10-45,
 * models/tacotron.py:9-43).  `tensors` hold the model's state_dict entries (fp32 [dev]). */
tts_status tts_tacotron_create(const tts_tacotron_config* cfg, const tts_tensor* tensors, int n_tensors,
                               void* stream, tts_tacotron** out);
void tts_tacotron_destroy(tts_tacotron* t);

/* Replaces the embedding + Encoder (Prenet + CBHG, layers/tacotron.py:209-243) +
 * _add_speaker_embedding + GST add of TacotronGST.inference (models/tacotrongst.py:65-73):
 *   ids         [dev]  int32 [B][Lmax]
 *   lens        [host] int32 [B], 1 <= lens[b] <= Lmax
 *   speaker_ids [host] int32 [B] or NULL
 *   style_mel   [dev]  fp32 [B][style_frames][80] or NULL (GST models only)
 *   out         [dev]  fp32 [B][Lmax][256], every sentence encoded at its own length, rows past
 *                      lens[b] zero (+0.0, every bit clear).
 * Padding contract of ids: entries ids[b][t], t >= lens[b], are never read as table rows and may
 * hold anything (negative values and values past the table included); Lmax may exceed the longest
 * lens[b].  Entries t < lens[b] must be rows of embedding.weight.  A speaker id outside
 * [0, num_speakers), style_mel on a model without GST, style_frames < 1 with style_mel, a lens[b]
 * outside [1, Lmax] or B / Lmax above the handle's capacity return TTS_ERR_INVALID and leave out
 * untouched.  speaker_ids are ignored by a model with num_speakers <= 1. */
tts_status tts_tacotron_encode(tts_tacotron* t, const int32_t* ids, const int32_t* lens, int B, int Lmax,
                               const int32_t* speaker_ids, const float* style_mel, int style_frames, float* out,
                               void* stream);
/* Which convolution kernel served each launch of the last tts_tacotron_encode (no reference
 * counterpart; the values of tts_postnet_last_path): kinds[0..9] = prenet layers 1, 2, the conv
 * bank, projections 1, 2, highways 1-4, the BiGRU input projection; kinds[10] = the GST GRU input
 * projection, -1 if the call had no style_mel.  n >= 11; -1 before the first call.  3 (16-frame
 * tiles) up to sum lens[b] = 4096 frames, 8 (64-frame tiles) above. */
tts_status tts_tacotron_encode_last_path(tts_tacotron* t, int* kinds, int n);

/* Replaces Decoder.inference (layers/tacotron.py:439-470) for a padded batch with per-sentence
 * batch-1 semantics (the reference's stop rule is batch-1, :464-469):
 *   enc [dev] fp32 [B][Lmax][256]; lens [host] int32 [B] (>= 1)
 *   mel [dev] fp32 [B][steps_cap*r][80]; stop [dev] fp32 [B][steps_cap] (sigmoid stop token);
 *   align [dev] fp32 [B][steps_cap][Lmax] or NULL; n_steps [host] int32 [B] out.
 * steps_cap >= max_steps + 1 (the reference stops once t > max_decoder_steps).
 * Padding contract of enc: rows enc[b][j], j >= lens[b], are never read into a result and may hold
 * anything (NaN included) on both serving paths: every use of them and of their input projection is
 * selected by j < lens[b], never multiplied by a zero weight.  Lmax may exceed the longest lens[b];
 * alignment columns j >= lens[b] are written as zero. */
tts_status tts_tacotron_decode(tts_tacotron* t, const float* enc, const int32_t* lens, int B, int Lmax,
                               int max_steps, int steps_cap, float* mel, float* stop, float* align,
                               int32_t* n_steps, void* stream);

/* Replaces Decoder.forward(inputs, memory, mask) (layers/tacotron.py:406-437) in eval mode: step t
 * decodes from memory_init (t = 0), then the queue updated with teacher row t-1 (80*r values); no stop
 * rule, exactly `steps` steps per sentence, each at its own encoder length.
 *   memories [dev] fp32 [B][mem_ldb], row t at t*80*r;  mel [dev] fp32 [B][steps][80*r];
 *   stop [dev] fp32 [B][steps] stopnet LOGITS;  align [dev] fp32 [B][steps][Lmax] or NULL.
 * steps <= max_steps + 1 (the history capacity); mem_ldb >= (steps - 1) * 80 * r: teacher rows
 * 0 .. steps-2 are read, the last row feeds no step and is never touched (it may be absent).  Every attention configuration and memory_size; always the multi-launch path
 * (tts_tacotron_last_path reports 0).  Returns after the steps have run. */
tts_status tts_tacotron_decode_teacher(tts_tacotron* t, const float* enc, const int32_t* lens, int B, int Lmax,
                                       const float* memories, int64_t mem_ldb, int steps, float* mel,
                                       float* stop, float* align, void* stream);

/* Replaces PostCBHG + last_linear + sigmoid (layers/tacotron.py:246-259, models/tacotrongst.py:43-45,
 * 77-78): mel [dev] fp32 [B][Tmax][80], T [host] int32 [B] -> linear [dev] fp32 [B][Tmax][1025]
 * (rows past T[b] zero).  Rows t >= T[b] of mel are never read and may hold anything (NaN
 * included); T[b] = 0 is legal and Tmax may exceed the longest T[b]. */
tts_status tts_tacotron_postnet(tts_tacotron* t, const float* mel, const int32_t* T, int B, int Tmax,
                                float* linear, void* stream);

tts_status tts_tacotron_last_timing(tts_tacotron* t, float* loop_ms, int* steps_run);

/* Which implementation ran the last tts_tacotron_decode (no reference counterpart): *resident = 1
 * for the resident single-launch decoder (each XCD holds the step weights on its 32 compute units
 * and decodes up to 4 sentences; hand-offs stay inside the XCD), 0 for the per-step multi-launch
 * hipGraph path.  The resident path serves B <= 32, Lmax <= 256, a memory queue of
 * 80 * memory_size <= 512 values (r <= memory_size <= 6), max_steps <= 1000 under
 * config_tacotron_gst.json's attention (sigmoid norm, forward attention without the eval mask, no
 * transition agent / location / windowing) on a GPU with >= 256 compute units; TTS_RESIDENT=0 in
 * the environment at tts_tacotron_create disables it.  A resident run whose hand-off wait timed
 * out re-runs the batch on the multi-launch path (reported 0). */
tts_status tts_tacotron_last_path(tts_tacotron* t, int* resident);

/* Measurement only: re-runs the last resident tts_tacotron_decode batch with phase timers and
 * returns the mean microseconds per decoder step of each phase on compute units 0 (the attention
 * leader of sentence 0) and 1 (a non-leader) of XCD 0: us[0..15] and us[16..31] (n >= 32):
 * 0 wait prenet-1 + continue flags, 1 prenet-2 rows + gather, 2 attention-GRU unit + gather, 3 query
 * rows + gather, 4 energies / weights / context partial, 5 leader: slice sums + publish, 6 gather
 * contexts, 7 alignment + project_to_decoder_in + gather, 8 decoder GRU 1 + gather, 9 GRU 2 +
 * gather, 10 mel rows + gather, 11 prenet-1 rows + stopnet; 12-15 split the compute (up to the
 * publish) out of 2, 8, 9 and 10. */
#define TTS_TACOTRON_RESIDENT_PHASES 16
tts_status tts_tacotron_resident_phases(tts_tacotron* t, float* us, int n);

/* Measurement only: mean duration (ms) of each decoder-step kernel over up to `reps` eager steps
 * of the last decode's batch, HIP events on the library stream, in launch order: prenet2,
 * attention GRU, query, attention, project_to_decoder_in, decoder GRU 1, decoder GRU 2, mel,
 * [prenet1 | stopnet]. */
#define TTS_TACOTRON_STEP_KERNELS 9
tts_status tts_tacotron_profile(tts_tacotron* t, int reps, float* kernel_ms, int n_kernels);

/* ---------------------------------------------------------------- evaluation losses
 * The criteria of train.py:462-465 as evaluate() applies them (train.py:327-339), on tensors that stay in
 * HBM: one read of every valid element of both operands, no masked copies, three numbers out.  The handle
 * carries the partials workspace: one fp64 partial per 8192-element chunk of work, grown on demand. */
typedef struct tts_loss tts_loss;
tts_status tts_loss_create(tts_loss** out);
void tts_loss_destroy(tts_loss* l);

#define TTS_LOSS_L1 0   /* L1LossMasked (layers/losses.py:7-33); nn.L1Loss when lengths is NULL   */
#define TTS_LOSS_MSE 1  /* MSELossMasked (layers/losses.py:36-62); nn.MSELoss when lengths is NULL */

/* Replaces sequence_mask + input * mask + target * mask + l1_loss / mse_loss (reduction="sum") + mask.sum()
 * + the division (layers/losses.py:27-33, 56-62; five passes over [B][T][D] and three tensors of that size
 * in the reference), and nn.L1Loss() / nn.MSELoss() (train.py:464) when lengths is NULL (every row counts).
 *   input, target [dev]  fp32 [B][T][D], rows contiguous (T * D floats per sentence), sentence b at
 *                        b * pitch elements: a decoder output view need not be contiguous over B
 *   lengths       [host] int32 [B] or NULL; sentence b contributes rows t < min(lengths[b], T)
 *   per_sentence  [dev]  fp64 [B] out: each sentence's sum of |x - y| or (x - y)^2 (0 without valid rows)
 *   loss_dev      [dev]  fp32 out: *loss_out rounded once
 *   sum_out, count_out, loss_out [host] out: the sum over all sentences, the number of terms
 *                        D * sum_b min(lengths[b], T) (mask.sum() as an integer), and sum / count; a count
 *                        of 0 gives NaN, as the reference's 0 / 0 does
 * The difference, its absolute value or square and every accumulation are fp64, from the fp32 operands.
 * The summation order is a function of the element index alone (wave reduction, one fp64 partial per
 * chunk, a second launch that folds the partials; no floating-point atomics, no hand-off inside a
 * launch), so the results are bitwise the same run to run and for any pitches and base addresses.
 * Rows at and beyond a sentence's length are NOT READ: they are padding, and at D = 1025 they are half the
 * traffic of a ragged batch.  One consequence differs from the reference: a NaN in the padding does not
 * reach the result here, while the reference's NaN * 0 does.
 * INVALID before any launch, outputs untouched: a null pointer (lengths excepted), a kind that is neither,
 * B, T or D <= 0, a pitch below T * D, a negative length.  Waits for the stream before it returns. */
tts_status tts_loss_masked(tts_loss* l, int kind, const float* input, int64_t input_pitch, const float* target,
                           int64_t target_pitch, const int32_t* lengths, int B, int T, int D, double* per_sentence,
                           float* loss_dev, double* sum_out, int64_t* count_out, double* loss_out, void* stream);

/* Replaces nn.BCEWithLogitsLoss() with its defaults on the stop logits (train.py:327, 465): the mean over
 * the n values of max(x, 0) - x y + log1p(exp(-|x|)), in fp64 from the fp32 operands, by the same two
 * launches (exp's argument is never positive: nothing overflows at any |x|).
 *   logits, targets [dev] fp32 [n]; sum_dev [dev] fp64 out: the sum; loss_dev [dev] fp32 out: *loss_out
 *   rounded once; sum_out, loss_out [host] out: the sum and sum / n.
 * INVALID before any launch: a null pointer, n <= 0.  Waits for the stream before it returns. */
tts_status tts_loss_bce_logits(tts_loss* l, const float* logits, const float* targets, int64_t n, double* sum_dev,
                               float* loss_dev, double* sum_out, double* loss_out, void* stream);

#define TTS_LOSS_BCE 2  /* nn.BCEWithLogitsLoss, for the gradient only: the forward has its own entry point */

/* The gradient of the five criteria with respect to input, for the loss.backward() of train.py:157: what
 * autograd derives from layers/losses.py:30-32, 59-61 (input * mask, the summed loss, the division by
 * mask.sum()) and from nn.L1Loss / nn.MSELoss / nn.BCEWithLogitsLoss, as one elementwise pass.  No handle:
 * the call has no workspace and no host staging, so it shares nothing with a forward in flight.
 *   input, target [dev]  fp32, B sentences of per_sentence = T * D elements, sentence b at b * pitch
 *   n_valid       [dev]  int64 [B]: sentence b's valid elements min(lengths[b], T) * D, clamped on the device
 *                        to [0, per_sentence]; NULL: per_sentence each (the plain criteria; BCE, with the
 *                        logits cut into B equal runs of any length, e.g. one per row)
 *   count         the forward's number of terms (the sum of n_valid), known to the host
 *   grad_output   [dev]  one fp32, the upstream gradient autograd hands over, or NULL: 1.  Read on the device.
 *   grad_input    [dev]  fp32 out, sentence b at b * grad_pitch
 * A valid element (index < n_valid[b]) is formed in fp64 from the fp32 operands and rounded to fp32 once:
 *   L1   grad_output * sign(x - y) / count, sign(0) = 0 as torch's l1_loss backward
 *   MSE  grad_output * 2 (x - y) / count
 *   BCE  grad_output * (sigmoid(x) - y) / count, the sigmoid as 1 / (1 + e^-x) for x >= 0 and
 *        e^x / (1 + e^x) otherwise: nothing overflows
 * Every element from n_valid[b] up to per_sentence is written +0.0; nothing between per_sentence and
 * grad_pitch is written; input and target are NOT READ at or beyond n_valid[b].  With count = 0 every
 * element of [B][per_sentence] is written NaN: the reference's 1 / mask.sum() is inf, and inf * 0 is NaN.
 * INVALID before any launch: a null input, target or grad_input, an unknown kind, B or per_sentence <= 0, a
 * pitch below per_sentence, a negative count.  One launch; does not wait for the stream and copies nothing
 * to the host. */
tts_status tts_loss_backward(int kind, const float* input, int64_t input_pitch, const float* target,
                             int64_t target_pitch, const int64_t* n_valid, int B, int64_t per_sentence, int64_t count,
                             const float* grad_output, float* grad_input, int64_t grad_pitch, void* stream);

/* ---------------------------------------------------------------- training update
 * The tail of every training iteration (train.py:157-167) on parameters, gradients and Adam state that stay
 * in HBM: the custom weight decay, clip_grad_norm_ and torch.optim.Adam.step (weight_decay = 0, no amsgrad),
 * as one fp64 norm reduction (two launches, as tts_loss_masked) and one pass that reads p, g, m, v once and
 * writes p, m, v once (g too when the clip scales it).  The forward and the backward stay the caller's torch.
 * The handle carries the chunk map of the tensor sizes (one chunk = TTS_OPTIM_CHUNK elements of one tensor,
 * one fp64 partial each), the device copy of the per-call table and its pinned host copies. */
typedef struct tts_optim tts_optim;
#define TTS_OPTIM_CHUNK 8192

/* One tensor of a call.  All pointers [dev] fp32, contiguous, numel elements.
 *   g     may be NULL (param.grad is None): the tensor does not count in the norm and is neither clipped nor
 *         stepped, as torch skips it; the weight decay still applies (generic_utils.py:178-181 tests nothing)
 *   m, v  exp_avg, exp_avg_sq; needed by tts_optim_adam and tts_optim_step only
 *   step  the number of THIS update (torch's state["step"] after its increment, >= 1); per tensor, as a
 *         tensor without a gradient does not advance; read by tts_optim_adam and tts_optim_step only */
typedef struct tts_optim_tensor {
    float* p;
    float* g;
    float* m;
    float* v;
    int64_t numel;
    int64_t step;
} tts_optim_tensor;

tts_status tts_optim_create(tts_optim** out);
void tts_optim_destroy(tts_optim* o);

/* The sizes of the tensor set: builds the chunk map (host, then one upload; waits for the stream).  Calling
 * it again with other sizes rebuilds it.  Every other call checks its table against these sizes.
 * INVALID: a null pointer, n <= 0, an element count <= 0. */
tts_status tts_optim_set_tensors(tts_optim* o, const int64_t* numel, int n, void* stream);

/* The total gradient norm of clip_grad_norm_(parameters, max_norm) (generic_utils.py:158), nothing scaled.
 *   norm64_dev [dev] fp64 [2] out: the sum of g * g over every element of every tensor with a gradient
 *              (products and sums in fp64 from the fp32 operand, fixed order), and its square root
 *   norm32_dev [dev] fp32 [2] out: the norm rounded once; the clip coefficient float(max_norm / (norm + 1e-6))
 *              where that fp64 quotient is below 1, else exactly 1.0f (a NaN quotient stays NaN)
 *   sumsq_out, norm_out [host] out, each may be NULL; if either is given the call waits for the stream
 * The table goes up on the stream from pinned memory with every call.  INVALID before any launch, outputs
 * untouched: a null handle, table or device output; n <= 0 or not the n of the sizes set; an element count
 * <= 0 or not the one set; a null p; two entries with the same p; max_norm <= 0. */
tts_status tts_optim_grad_norm(tts_optim* o, const tts_optim_tensor* t, int n, double max_norm, double* norm64_dev,
                               float* norm32_dev, double* sumsq_out, double* norm_out, void* stream);

/* Replaces torch.nn.utils.clip_grad_norm_ in check_update (generic_utils.py:155-162): tts_optim_grad_norm,
 * then g <- g * coefficient in place where the coefficient is not 1.0f.  Arguments and checks as above. */
tts_status tts_optim_clip(tts_optim* o, const tts_optim_tensor* t, int n, double max_norm, double* norm64_dev,
                          float* norm32_dev, double* sumsq_out, double* norm_out, void* stream);

/* Replaces weight_decay(optimizer, wd) (generic_utils.py:174-182): p <- p + float(-wd * lr) * p, in place, on
 * every tensor (m, v, g are not read and may be NULL).  wd == 0 launches nothing.
 * INVALID: the table checks above; lr <= 0. */
tts_status tts_optim_decay(tts_optim* o, const tts_optim_tensor* t, int n, double lr, double wd, void* stream);

/* Replaces optimizer.step() of torch.optim.Adam(lr, betas, eps, weight_decay=0) (train.py:160, 454-457) as
 * torch/optim/adam.py::_single_tensor_adam computes it: m <- m + w1 (g - m); v <- v * beta2, v <- v + (w2 g) g;
 * p <- p + (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps), fp32, one rounding per operation, with
 * w1 = 1 - beta1, w2 = 1 - beta2, bc = 1 - beta^step in double and each scalar rounded once.
 * INVALID: the table checks above; a null m or v or a step < 1 on a tensor with a gradient; lr <= 0; a beta
 * outside [0, 1); eps < 0. */
tts_status tts_optim_adam(tts_optim* o, const tts_optim_tensor* t, int n, double lr, double beta1, double beta2,
                          double eps, void* stream);

/* The three of train.py:158-160 in one pass over the parameter set: the norm (two launches), then per
 * element decay, clip, Adam in that order, the clip coefficient read from norm32_dev[1] on the device (the
 * host waits for nothing).  Bitwise tts_optim_decay, tts_optim_clip, tts_optim_adam in sequence.
 * INVALID: the union of their checks. */
tts_status tts_optim_step(tts_optim* o, const tts_optim_tensor* t, int n, double lr, double beta1, double beta2,
                          double eps, double wd, double max_norm, double* norm64_dev, float* norm32_dev,
                          void* stream);

/* ---------------------------------------------------------------- trainable LSTM
 * The encoder's nn.LSTM(512, 256, num_layers=1, batch_first=True, bidirectional=True) as Encoder.forward
 * runs it on a packed batch (layers/tacotron2.py:56-76), with its whole backward: one layer, one or two
 * directions, gate rows i, f, g, o, fp32, biases on, no dropout, no projection.  Every product is an exact
 * fp32 MFMA chain, every reduction has a fixed order and nothing is accumulated with atomics: the same
 * operands give the same bits.  The handle owns the repacked weights and the workspaces (the input
 * projection, dpre, the carried cell state and cell gradient, the weight-gradient partials), grown on
 * demand; all calls on one handle must be ordered on one stream.  The reserve (what the forward keeps for
 * the backward) belongs to the caller, so several forwards may be outstanding before their backwards.
 * No call waits for the stream or copies to or from the host (the lengths travel as kernel arguments); a
 * workspace that has to grow is freed and allocated again, which waits for the device that once.
 * Every [dev] tensor must be 16-byte aligned. */
typedef struct tts_lstm tts_lstm;

/* UNSUPPORTED unless input_size and hidden_size are positive multiples of 16. */
tts_status tts_lstm_create(int input_size, int hidden_size, int bidirectional, tts_lstm** out);
void tts_lstm_destroy(tts_lstm* l);

/* The parameters of direction d (0: weight_ih_l0 ..., 1: the _reverse set; [1] is not read without the second
 * direction), [dev] in nn.LSTM's layout: w_ih [4H][I], w_hh [4H][H], b_ih, b_hh [4H].  Repacks them on the
 * stream into the orders the kernels read; call it again whenever the parameters have changed. */
tts_status tts_lstm_set_weights(tts_lstm* l, const float* const* w_ih, const float* const* w_hh,
                                const float* const* b_ih, const float* const* b_hh, void* stream);

/* Floats of the reserve a forward of this shape fills: the four activated gates and c_t of every position,
 * and a copy of the initial cell state.  0 for a null handle or a B or Tmax <= 0. */
int64_t tts_lstm_reserve_floats(const tts_lstm* l, int B, int Tmax);

/* Replaces pack_padded_sequence + self.lstm + pad_packed_sequence (layers/tacotron2.py:68-75), and the
 * padded calls of Encoder.inference / inference_truncated (:82, :92) with every length = Tmax.
 *   x        [dev]  [B][Tmax][I]; rows t >= lens[b] are NOT READ
 *   lens     [host] int32 [B], 1 <= lens[b] <= Tmax, in any order
 *   h0, c0   [dev]  [D][B][H] or NULL (zeros)
 *   out      [dev]  [B][Tmax][D * H] = [h_fwd(t) | h_bwd(t)]; rows t >= lens[b] are written +0.0
 *   h_n, c_n [dev]  [D][B][H] or NULL: each direction's state after its last valid position
 *   reserve  [dev]  tts_lstm_reserve_floats(l, B, Tmax) floats, or NULL (no backward will follow: nothing
 *                   extra is stored, and out is bitwise the same)
 * INVALID before any launch: a null handle, x, lens or out; weights not set; B or Tmax <= 0; a length
 * outside [1, Tmax]; a misaligned tensor.  2 + 2 launches, then one per time step up to max(lens). */
tts_status tts_lstm_forward(tts_lstm* l, const float* x, const int32_t* lens, int B, int Tmax, const float* h0,
                            const float* c0, float* out, float* h_n, float* c_n, float* reserve, void* stream);

/* The backward of that forward for an upstream gradient of out (autograd's walk back through
 * layers/tacotron2.py:68-75; no gradient flows into h_n, c_n or out of h0, c0).
 *   x, lens, B, Tmax, h0   as the forward had them; reserve, out: what it wrote
 *   grad_out  [dev]  [B][Tmax][D * H]; rows t >= lens[b] are NOT READ
 *   grad_x    [dev]  [B][Tmax][I] out, summed over the directions; rows t >= lens[b] are written +0.0
 *   grad_w_ih, grad_w_hh, grad_b_ih, grad_b_hh  [2] of [dev] out in the parameters' layouts, sums over the
 *             valid positions only ([1] is not read without the second direction)
 * Gradients are WRITTEN, not accumulated.  grad_x, any of the four arrays and any entry of one may be NULL;
 * that product is skipped.  The weights are those of the last tts_lstm_set_weights: they must be the
 * forward's.  INVALID before any launch: as the forward; a null reserve, out or grad_out.  2 launches, one
 * per time step, then at most 12. */
tts_status tts_lstm_backward(tts_lstm* l, const float* x, const int32_t* lens, int B, int Tmax, const float* reserve,
                             const float* out, const float* h0, const float* grad_out, float* grad_x,
                             float* const* grad_w_ih, float* const* grad_w_hh, float* const* grad_b_ih,
                             float* const* grad_b_hh, void* stream);

/* ---------------------------------------------------------------- trainable conv-BN block (convbn_train.hip)
 * The reference's ConvBNBlock (layers/tacotron2.py:9-27): Conv1d(k = 5, padding = 2) -> BatchNorm1d ->
 * ReLU | Tanh | nothing -> Dropout, as Encoder.convolutions (:52-55) and Postnet.convolutions (:30-45) run it
 * in training, with its whole backward; with training == 0 it normalises with the running statistics.
 * Every product is an exact fp32 MFMA chain, the per-channel sums are fp64 partials folded in a fixed order,
 * nothing is accumulated with atomics: the same operands give the same bits.  The handle owns the repacked
 * weights and the workspaces, grown on demand; all calls on one handle must be ordered on one stream.  The
 * reserve belongs to the caller, so several forwards may be outstanding before their backwards.  No call
 * waits for the stream or copies to or from the host; a workspace that has to grow is freed and allocated
 * again, which waits for the device that once.  Activations are [B][C][T] contiguous fp32 with 4-byte
 * alignment only; T is arbitrary. */
typedef struct tts_convbn tts_convbn;

/* act: 0 none, 1 relu, 2 tanh (else INVALID).  UNSUPPORTED unless kernel_size == 5 and cin, cout are positive
 * multiples of 16. */
tts_status tts_convbn_create(int cin, int cout, int kernel_size, int act, tts_convbn** out);
void tts_convbn_destroy(tts_convbn* h);

/* [dev] W [cout][cin][5] (net.0.weight), bias [cout] (net.0.bias), gamma, beta [cout] (net.1.weight, .bias).
 * Repacks W on the stream for the forward, grad_x (taps flipped, transposed) and keeps copies of the three
 * vectors; call it again whenever the parameters have changed. */
tts_status tts_convbn_set_weights(tts_convbn* h, const float* W, const float* bias, const float* gamma,
                                  const float* beta, void* stream);

/* Floats of the reserve a training forward of this shape fills: y = conv(x) + bias [B][cout][T], the batch
 * mean and 1 / sqrt(var + eps) per channel, the dropout scale.  0 for a null handle or a B or T <= 0. */
int64_t tts_convbn_reserve_floats(const tts_convbn* h, int B, int T);

/* self.net(x) (layers/tacotron2.py:25-27).
 *   x        [dev]  [B][cin][T]
 *   mask     [dev]  uint8 [B][cout][T], 1 = keep (training only; not read otherwise)
 *   p_keep_scale    1 / (1 - p) of the dropout (training only)
 *   running_mean, running_var [dev] [cout]: training: updated in place with `momentum` (the variance
 *            unbiased, n / (n - 1)); else the statistics that normalise
 *   out      [dev]  [B][cout][T]; an element with mask == 0 is +0.0
 *   reserve  [dev]  tts_convbn_reserve_floats(h, B, T) floats, or NULL (no backward will follow; out is bitwise
 *            the same); not used with training == 0
 * Batch statistics run over all B * T positions of a channel (biased variance).
 * INVALID before any launch, with nothing written: a null handle, x, out or running buffer; weights not set;
 * B or T <= 0; in training a null mask or B * T == 1.  5 launches in training, 4 otherwise. */
tts_status tts_convbn_forward(tts_convbn* h, const float* x, int B, int T, const uint8_t* mask, float p_keep_scale,
                              float* running_mean, float* running_var, double momentum, double eps, int training,
                              float* out, float* reserve, void* stream);

/* The backward of that training forward for an upstream gradient of out.
 *   x, B, T, mask  as the forward had them; reserve: what it wrote
 *   grad_out [dev]  [B][cout][T]
 *   grad_x   [dev]  [B][cin][T];  grad_W [cout][cin][5];  grad_bias, grad_gamma, grad_beta [cout]
 * Gradients are WRITTEN, not accumulated.  Any of the five may be NULL; that product is skipped.  The weights
 * are those of the last tts_convbn_set_weights: they must be the forward's.  INVALID before any launch: as
 * the forward; a null reserve, mask or grad_out.  At most 10 launches. */
tts_status tts_convbn_backward(tts_convbn* h, const float* x, int B, int T, const float* reserve, const uint8_t* mask,
                               const float* grad_out, float* grad_x, float* grad_W, float* grad_bias, float* grad_gamma,
                               float* grad_beta, void* stream);

/* ---------------------------------------------------------------- trainable Tacotron2 decoder (decoder_train.hip)
 * The reference's Decoder (layers/tacotron2.py:97-247) as Decoder.forward runs it teacher-forced, with its whole
 * backward through time: prenet ("original"), attention LSTM cell, attention (no location term, no transition
 * agent; "sigmoid" or "softmax" norm, forward attention with u = 0.5 or none), decoder LSTM cell, projection,
 * stopnet (separate: reads its input detached; else its input gradient joins).  Every product is an exact fp32
 * MFMA chain, every reduction has a fixed order and nothing is accumulated with atomics: the same operands and
 * masks give the same bits.  Plain launches on the caller's stream; no call waits for the stream or copies to or
 * from the host; a workspace that has to grow is freed and allocated again, which waits for the device that
 * once.  The handle owns the repacked weights (transposed copies included) and the workspaces; all calls on one
 * handle must be ordered on one stream.  The reserve belongs to the caller, so several forwards may be
 * outstanding before their backwards.  [dev] tensors are contiguous fp32 with 4-byte alignment, the reserve
 * 16-byte.
 *
 * Shapes: B sentences, L text positions, T decoder steps (= mel frames / r), MR = mel * r.
 * Dropout masks are operands: uint8, 1 = keep, step-major ([T][B][...]: step t of sentence b is row t * B + b). */
typedef struct tts_dectrain tts_dectrain;

/* The reference's parameter tensors by name, [dev], in the reference's layouts. */
typedef struct {
    const float* prenet_w1; /* prenet.layers.0.linear_layer.weight            [prenet][MR] */
    const float* prenet_w2; /* prenet.layers.1.linear_layer.weight            [prenet][prenet] */
    const float* att_w_ih;  /* attention_rnn.weight_ih                        [4 rnn][prenet + enc] */
    const float* att_w_hh;  /* attention_rnn.weight_hh                        [4 rnn][rnn] */
    const float* att_b_ih;  /* attention_rnn.bias_ih                          [4 rnn] */
    const float* att_b_hh;  /* attention_rnn.bias_hh                          [4 rnn] */
    const float* query_w;   /* attention_layer.query_layer.linear_layer.weight  [att][rnn] */
    const float* inputs_w;  /* attention_layer.inputs_layer.linear_layer.weight [att][enc] */
    const float* v_w;       /* attention_layer.v.linear_layer.weight          [1][att] */
    const float* v_b;       /* attention_layer.v.linear_layer.bias            [1] */
    const float* dec_w_ih;  /* decoder_rnn.weight_ih                          [4 rnn][rnn + enc] */
    const float* dec_w_hh;  /* decoder_rnn.weight_hh                          [4 rnn][rnn] */
    const float* dec_b_ih;  /* decoder_rnn.bias_ih                            [4 rnn] */
    const float* dec_b_hh;  /* decoder_rnn.bias_hh                            [4 rnn] */
    const float* proj_w;    /* linear_projection.linear_layer.weight          [MR][rnn + enc] */
    const float* proj_b;    /* linear_projection.linear_layer.bias            [MR] */
    const float* stop_w;    /* stopnet.1.linear_layer.weight                  [1][rnn + MR] */
    const float* stop_b;    /* stopnet.1.linear_layer.bias                    [1] */
    const float* att_init;  /* attention_rnn_init.weight                      [1][rnn] */
    const float* go_init;   /* go_frame_init.weight                           [1][MR] */
    const float* dec_init;  /* decoder_rnn_inits.weight                       [1][rnn] */
} tts_dectrain_weights;

/* The same table for the gradients, [dev] out in the parameters' layouts; any entry may be NULL (skipped). */
typedef struct {
    float *prenet_w1, *prenet_w2, *att_w_ih, *att_w_hh, *att_b_ih, *att_b_hh, *query_w, *inputs_w, *v_w, *v_b, *dec_w_ih,
        *dec_w_hh, *dec_b_ih, *dec_b_hh, *proj_w, *proj_b, *stop_w, *stop_b, *att_init, *go_init, *dec_init;
} tts_dectrain_grads;

/* The four groups of dropout masks of a training forward and their scales 1 / (1 - p). */
typedef struct {
    const uint8_t* prenet1; /* [T][B][prenet] after the first prenet layer  (prenet_dropout only) */
    const uint8_t* prenet2; /* [T][B][prenet] after the second */
    const uint8_t* att_h;   /* [T][B][rnn] on the attention LSTM's h */
    const uint8_t* att_c;   /* [T][B][rnn] on its cell state: the dropped tensors are the carried state */
    const uint8_t* dec_h;   /* [T][B][rnn] decoder LSTM */
    const uint8_t* dec_c;   /* [T][B][rnn] */
    const uint8_t* stop;    /* [T][B][rnn + MR] on the stopnet's input [h_dec | decoder_output] */
    float scale_prenet, scale_rnn, scale_stop;
} tts_dectrain_masks;

/* norm: 0 "sigmoid", 1 "softmax" (else INVALID).  UNSUPPORTED unless enc, prenet, rnn and att are positive
 * multiples of 16 and mel_r is positive. */
tts_status tts_dectrain_create(int enc, int prenet, int rnn, int att, int mel_r, int norm, int forward_attn,
                               int prenet_dropout, int separate_stopnet, tts_dectrain** out);
void tts_dectrain_destroy(tts_dectrain* h);

/* Repacks the parameters on the stream into the orders the kernels read (gate-interleaved rows for the two
 * cells' forward, transposed copies for the backward, mel * r padded to 16); call it again whenever the
 * parameters have changed.  INVALID: a null entry. */
tts_status tts_dectrain_set_weights(tts_dectrain* h, const tts_dectrain_weights* w, void* stream);

/* Floats of the reserve a forward of this shape fills: both cells' h of every step (and the initial rows), the
 * contexts, alpha, the queries, both cells' activated gates and cell states, the prenet's two outputs, the
 * frames, decoder_output, the processed memory and the inputs with +0.0 on masked rows.  0 for a null handle or
 * a non-positive B, L or T. */
int64_t tts_dectrain_reserve_floats(const tts_dectrain* h, int B, int L, int T);

/* Decoder.forward(inputs, memories, mask) (layers/tacotron2.py:227-247).
 *   inputs     [dev]  [B][L][enc]; a row with mask == 0 never reaches a product (selected away)
 *   memories   [dev]  [B][T * r][mel] the teacher's frames; the last group of r frames is not read
 *   mask       [dev]  uint8 [B][L], 1 = valid, or NULL (all valid).  The host never reads it; every sentence needs
 *                     one valid position (not checked: undefined otherwise, as in the reference)
 *   training   1: the masks of m drop (all but prenet1 / prenet2 required; those with prenet_dropout); 0: m is not
 *              read and nothing is dropped
 *   out        [dev]  [B][T][MR] decoder_output (the reference's outputs is its view [B][T * r][mel] transposed)
 *   stop       [dev]  [B][T];  alignments [dev] [B][T][L]
 *   reserve    [dev]  tts_dectrain_reserve_floats(h, B, L, T) floats, or NULL (no backward will follow: the handle's
 *                     own block is used and the outputs are bitwise the same)
 * INVALID before any launch: a null handle or tensor; weights not set; B, L or T <= 0; L > 2048 or
 * 4 * ceil16(L) + enc + 512 floats above the 64 KB of LDS the attention kernels may ask for; training
 * without its masks or with a scale <= 0; a misaligned reserve.  10 launches, 4 per step, 3. */
tts_status tts_dectrain_forward(tts_dectrain* h, const float* inputs, const float* memories, const uint8_t* mask, int B,
                                int L, int T, int training, const tts_dectrain_masks* m, float* out, float* stop,
                                float* alignments, float* reserve, void* stream);

/* The backward of that training forward.
 *   mask, B, L, T, m  as the forward had them; reserve: what it wrote
 *   grad_out   [dev]  [B][T][MR] or NULL (zeros);  grad_stop [dev] [B][T] or NULL (zeros); one of them is required.
 *              With a separate stopnet grad_stop reaches only stop_w and stop_b.
 *   grad_inputs [dev] [B][L][enc] (through the contexts and the processed memory; +0.0 on masked rows);
 *   grad_memories [dev] [B][T * r][mel] (+0.0 on the last group);  g: the parameters' gradients
 * Gradients are WRITTEN, not accumulated.  Any gradient pointer may be NULL; that product is skipped, and when
 * only stop_w / stop_b are asked for the walk back through time is skipped altogether.  The weights are those of
 * the last tts_dectrain_set_weights: they must be the forward's.  INVALID before any launch: as the forward; a
 * null reserve, m, g or mask group; neither grad_out nor grad_stop. */
tts_status tts_dectrain_backward(tts_dectrain* h, const uint8_t* mask, int B, int L, int T, const tts_dectrain_masks* m,
                                 const float* reserve, const float* grad_out, const float* grad_stop, float* grad_inputs,
                                 float* grad_memories, const tts_dectrain_grads* g, void* stream);

/* ---------------------------------------------------------------- trainable GRU (gru_train.hip)
 * The single-layer nn.GRU of the Tacotron / TacotronGST family with its whole backward: the CBHG's
 * nn.GRU(128, 128, 1, batch_first=True, bidirectional=True) of the encoder and the postnet
 * (layers/tacotron.py:165-170, :204-205; gradient of `outputs`) and the GST reference encoder's
 * nn.GRU(256, 128, batch_first=True) (layers/gst_layers.py:53-56, :74-78; gradient of h_n only).  One or two
 * directions, gate rows r, z, n, fp32, biases on, every sentence at full length T (the reference neither packs
 * nor masks here).  The cell is ATen's:
 *   xi = W_ih x_t + b_ih,  hh = W_hh h_prev + b_hh,
 *   r = s(xi_r + hh_r), z = s(xi_z + hh_z), n = tanh(xi_n + r * hh_n), h = (1 - z) * n + z * h_prev.
 * All arithmetic is fp32; every matrix product is an exact fp32 MFMA chain (v_mfma_f32_16x16x4_f32) in a fixed
 * k order (within a 16-k chunk k = 4g + j, the four g inside one MFMA, j over four MFMAs), every
 * reduction has a fixed order and nothing is accumulated with atomics: the same operands give the same bits,
 * forward and backward.  The recurrence of a forward is ONE launch, and so is that of a backward: a workgroup
 * per direction and 16 sentences walks all T steps with its rows of W_hh (W_hh^T) stationary in registers and
 * the previous state (the previous dpre_h) in LDS; no workgroup waits for another.  The launch count of a call
 * does not depend on T.  The handle owns the repacked weights and the workspaces (the input projection, dpre_i,
 * dpre_h, the weight-gradient partials), grown on demand; all calls on one handle must be ordered on one
 * stream.  The reserve belongs to the caller, so several forwards may be outstanding before their backwards.
 * No call waits for the stream or copies to or from the host; a workspace that has to grow is freed and
 * allocated again, which waits for the device that once.  Every [dev] tensor must be 16-byte aligned.
 * Diagnostic switch: with TTS_GRU_STEPWISE=1 in the environment when the handle is created, its calls launch the
 * two recurrence kernels once per time step (the state travels through out, dpre_h and a carry buffer; the same
 * bits).  It exists for the single-launch against per-step-launch comparison of tools/bench_gru_train.py. */
typedef struct tts_gru tts_gru;

/* UNSUPPORTED unless input_size is a positive multiple of 16 and hidden_size a positive multiple of 16 that
 * is <= 128 (a direction's W_hh has to fit one workgroup's registers). */
tts_status tts_gru_create(int input_size, int hidden_size, int bidirectional, tts_gru** out);
void tts_gru_destroy(tts_gru* g);

/* The parameters of direction d (0: weight_ih_l0 ..., 1: the _reverse set; [1] is not read without the second
 * direction), [dev] in nn.GRU's layout: w_ih [3H][I], w_hh [3H][H], b_ih, b_hh [3H].  Repacks them on the
 * stream; call it again whenever the parameters have changed. */
tts_status tts_gru_set_weights(tts_gru* g, const float* const* w_ih, const float* const* w_hh,
                               const float* const* b_ih, const float* const* b_hh, void* stream);

/* Floats of the reserve a forward of this shape fills: r, z, n and hh_n = W_hh_n h_prev + b_hh_n of every
 * position and direction, [B][T][D][4][H].  0 for a null handle or a B or T <= 0. */
int64_t tts_gru_reserve_floats(const tts_gru* g, int B, int T);

/* `outputs, h_n = gru(x)` (layers/tacotron.py:204-205, layers/gst_layers.py:76-77).
 *   x        [dev]  [B][T][I]
 *   h0       [dev]  [D][B][H] or NULL (zeros); a constant: no gradient is produced for it
 *   out      [dev]  [B][T][D * H] = [h_fwd(t) | h_bwd(t)]
 *   h_n      [dev]  [D][B][H] or NULL: the forward direction's state after t = T - 1, the reverse one's after 0
 *   reserve  [dev]  tts_gru_reserve_floats(g, B, T) floats, or NULL (no backward will follow: nothing extra
 *                   is stored, and out, h_n are bitwise the same)
 * INVALID before any launch: a null handle, x or out; weights not set; B or T <= 0; B * T >= 2^24; a
 * misaligned tensor.  2 launches: the input projection of both directions, the recurrence. */
tts_status tts_gru_forward(tts_gru* g, const float* x, int B, int T, const float* h0, float* out, float* h_n,
                           float* reserve, void* stream);

/* The backward of that forward.  dh_t = grad_out[:, t] + carry; the carry starts as grad_h_n:
 *   da_n = dh * (1 - z) * (1 - n^2),  da_z = dh * (h_prev - n) * z * (1 - z),  da_r = da_n * hh_n * r * (1 - r)
 *   dpre_i = [da_r | da_z | da_n]      grad_W_ih = dpre_i^T x,      grad_b_ih = sum dpre_i,  grad_x = dpre_i W_ih
 *   dpre_h = [da_r | da_z | da_n * r]  grad_W_hh = dpre_h^T h_prev, grad_b_hh = sum dpre_h
 *   carry  = dh * z + dpre_h W_hh
 *   x, B, T, h0   as the forward had them; reserve, out: what it wrote
 *   grad_out  [dev]  [B][T][D * H] or NULL;  grad_h_n [dev] [D][B][H] or NULL.  A NULL one is read as zero (it is
 *             not loaded at all); the result is bitwise that of the same call with zeros passed.
 *   grad_x    [dev]  [B][T][I] out, summed over the directions
 *   grad_w_ih, grad_w_hh, grad_b_ih, grad_b_hh  [2] of [dev] out in the parameters' layouts ([1] is not read
 *             without the second direction)
 * Gradients are WRITTEN, not accumulated.  grad_x, any of the four arrays and any entry of one may be NULL;
 * that product is skipped.  The weights are those of the last tts_gru_set_weights: they must be the forward's.
 * INVALID before any launch: as the forward; a null reserve or out; grad_out and grad_h_n both NULL.  One
 * launch for the recurrence, then at most 11 (column sums, the weight-gradient partials in row chunks of 512
 * folded in chunk order, grad_x). */
tts_status tts_gru_backward(tts_gru* g, const float* x, int B, int T, const float* reserve, const float* out,
                            const float* h0, const float* grad_out, const float* grad_h_n, float* grad_x,
                            float* const* grad_w_ih, float* const* grad_w_hh, float* const* grad_b_ih,
                            float* const* grad_b_hh, void* stream);

const char* tts_last_error(void);
const char* tts_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TTS_HIP_H */
