"""Drop-in for the reference ``AudioProcessor`` (utils/audio.py:11-255).

``inv_mel_spectrogram`` / ``inv_spectrogram`` keep the reference signatures (numpy [n, T] in,
numpy float64 waveform out) and run Griffin-Lim on the GPU through libtts_hip ``tts_gl_run``:
denormalise -> dB->amp -> pinv(mel basis) -> ^power -> GL (librosa 0.6.2 stft/istft semantics)
-> inverse pre-emphasis, all in HIP.  The initial phases are drawn on the host with
``np.random.rand(*S.shape)`` exactly as utils/audio.py:183 does, so a caller that seeds numpy gets
the same phases as the reference.  ``inv_mel_spectrogram_batch`` is the batched GPU-resident form
(torch tensors in HBM, device-drawn phases) the batched/sharded synthesis uses.

The analysis half runs on the GPU too: ``spectrogram`` / ``melspectrogram`` (``tts_gl_analyze``; both
from one STFT in ``features_batch``) and ``out_linear_to_mel`` (``tts_gl_linear_to_mel``), with batched
forms on torch tensors in the frame-major layout Griffin-Lim reads.  The reference's small helpers
(``_normalize``, ``mulaw_encode``, ``quantize``, ...) are restated in numpy on the host.

The mel filter bank is librosa 0.6.2 ``filters.mel`` (Slaney, area-normalised), restated in
numpy because librosa is not installed; its pseudo-inverse is computed once in float64 on the
host (utils/audio.py:64-66 recomputes it on every call).
"""
from __future__ import annotations

import contextlib
import ctypes
import io as _io

import numpy as np
import scipy.io.wavfile
import scipy.signal
import torch

from . import _native


def _hz_to_mel(f):
    f = np.atleast_1d(np.asarray(f, dtype=np.float64))
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    mel = f / f_sp
    hi = f >= min_log_hz
    mel[hi] = min_log_mel + np.log(f[hi] / min_log_hz) / logstep
    return mel


def _mel_to_hz(m):
    m = np.atleast_1d(np.asarray(m, dtype=np.float64))
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    f = f_sp * m
    hi = m >= min_log_mel
    f[hi] = min_log_hz * np.exp(logstep * (m[hi] - min_log_mel))
    return f


def mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa 0.6.2 filters.mel(sr, n_fft, n_mels, fmin, fmax), htk=False, norm=1."""
    fmax = float(sr) / 2 if fmax is None else fmax
    bins = np.linspace(0, float(sr) / 2, 1 + n_fft // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin)[0], _hz_to_mel(fmax)[0], n_mels + 2))
    lo, ce, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    rise = (bins[None, :] - lo) / (ce - lo)
    fall = (hi - bins[None, :]) / (hi - ce)
    w = np.maximum(0.0, np.minimum(rise, fall))
    return w * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def resample_filter(res_type="kaiser_best"):
    """resampy 0.2.x's interpolation filter by name: (half_win float64 [num_table * num_zeros + 1],
    num_table).  "kaiser_best" is sinc_window(num_zeros=64, precision=9, kaiser(beta=14.769656459379492),
    rolloff=0.9475937167399596), the filter librosa.load resamples with; no other name is built (a caller
    may hand resample_batch its own (half_win, num_table) pair)."""
    if res_type != "kaiser_best":
        raise NotImplementedError("resample filter %r (only 'kaiser_best' is built)" % (res_type,))
    num_zeros, precision, beta, rolloff = 64, 9, 14.769656459379492, 0.9475937167399596
    num_table = 2 ** precision
    n = num_table * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = scipy.signal.windows.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_table


def resample_lengths(N, orig_sr, target_sr):
    """(n_res, n_fix) of N samples resampled from orig_sr to target_sr: resampy's output length
    int(N * ratio) and librosa's fix_length int(ceil(N * ratio)); the result has n_fix samples, zero at and
    beyond n_res.  ValueError when n_res < 1, as resampy raises."""
    ratio = float(target_sr) / orig_sr
    n_res = int(N * ratio)
    if n_res < 1:
        raise ValueError("Input signal length=%d is too small to resample from %s->%s" % (N, orig_sr, target_sr))
    return n_res, int(np.ceil(N * ratio))


class AudioProcessor:
    def __init__(self, sample_rate=None, num_mels=None, min_level_db=None, frame_shift_ms=None,
                 frame_length_ms=None, ref_level_db=None, num_freq=None, power=None, preemphasis=None,
                 signal_norm=None, symmetric_norm=None, max_norm=None, mel_fmin=None, mel_fmax=None,
                 clip_norm=True, griffin_lim_iters=None, do_trim_silence=False, **kwargs):
        self.sample_rate = sample_rate
        self.num_mels = num_mels
        self.min_level_db = min_level_db
        self.frame_shift_ms = frame_shift_ms
        self.frame_length_ms = frame_length_ms
        self.ref_level_db = ref_level_db
        self.num_freq = num_freq
        self.power = power
        self.preemphasis = preemphasis
        self.griffin_lim_iters = griffin_lim_iters
        self.signal_norm = signal_norm
        self.symmetric_norm = symmetric_norm
        self.mel_fmin = 0 if mel_fmin is None else mel_fmin
        self.mel_fmax = mel_fmax
        self.max_norm = 1.0 if max_norm is None else float(max_norm)
        self.clip_norm = clip_norm
        self.do_trim_silence = do_trim_silence
        self.n_fft, self.hop_length, self.win_length = self._stft_parameters()
        self._gl = None
        self._mel_basis_set = False
        self._resample_filter = None  # the named resample filter the handle holds (None: none, or a caller's table)

    def _stft_parameters(self):  # utils/audio.py:114-119
        n_fft = (self.num_freq - 1) * 2
        hop_length = int(self.frame_shift_ms / 1000.0 * self.sample_rate)
        win_length = int(self.frame_length_ms / 1000.0 * self.sample_rate)
        return n_fft, hop_length, win_length

    def _build_mel_basis(self):  # utils/audio.py:68-77
        if self.mel_fmax is not None:
            assert self.mel_fmax <= self.sample_rate // 2
        return mel_basis(self.sample_rate, self.n_fft, self.num_mels, self.mel_fmin, self.mel_fmax)

    # ---------------------------------------------------------------- host helpers (not hot)
    def _denormalize(self, S):  # utils/audio.py:96-112
        if not self.signal_norm:
            return S
        if self.symmetric_norm:
            if self.clip_norm:
                S = np.clip(S, -self.max_norm, self.max_norm)
            return ((S + self.max_norm) * -self.min_level_db / (2 * self.max_norm)) + self.min_level_db
        if self.clip_norm:
            S = np.clip(S, 0, self.max_norm)
        return (S * -self.min_level_db / self.max_norm) + self.min_level_db

    def _db_to_amp(self, x):  # utils/audio.py:125-126
        return np.power(10.0, x * 0.05)

    def _linear_to_mel(self, spectrogram):  # utils/audio.py:60-62
        return np.dot(self._build_mel_basis(), spectrogram)

    def _mel_to_linear(self, mel_spec):  # utils/audio.py:64-66
        inv_mel_basis = np.linalg.pinv(self._build_mel_basis())
        return np.maximum(1e-10, np.dot(inv_mel_basis, mel_spec))

    def _normalize(self, S):  # utils/audio.py:79-94
        if not self.signal_norm:
            return S
        S_norm = ((S - self.min_level_db) / - self.min_level_db)
        if self.symmetric_norm:
            S_norm = ((2 * self.max_norm) * S_norm) - self.max_norm
            if self.clip_norm:
                S_norm = np.clip(S_norm, -self.max_norm, self.max_norm)
            return S_norm
        S_norm = self.max_norm * S_norm
        if self.clip_norm:
            S_norm = np.clip(S_norm, 0, self.max_norm)
        return S_norm

    def _amp_to_db(self, x):  # utils/audio.py:121-123
        min_level = np.exp(self.min_level_db / 20 * np.log(10))
        return 20 * np.log10(np.maximum(min_level, x))

    def apply_preemphasis(self, x):  # utils/audio.py:128-131
        if self.preemphasis == 0:
            raise RuntimeError(" !! Preemphasis is applied with factor 0.0. ")
        return scipy.signal.lfilter([1, -self.preemphasis], [1], x)

    @staticmethod
    def mulaw_encode(wav, qc):  # utils/audio.py:219-226
        mu = 2 ** qc - 1
        signal = np.sign(wav) * np.log(1 + mu * np.abs(wav)) / np.log(1. + mu)
        signal = (signal + 1) / 2 * mu + 0.5
        return np.floor(signal,)

    @staticmethod
    def mulaw_decode(wav, qc):  # utils/audio.py:228-233
        mu = 2 ** qc - 1
        return np.sign(wav) / mu * ((1 + mu) ** np.abs(wav) - 1)

    def encode_16bits(self, x):  # utils/audio.py:248-249
        return np.clip(x * 2**15, -2**15, 2**15 - 1).astype(np.int16)

    def quantize(self, x, bits):  # utils/audio.py:251-252
        return (x + 1.) * (2**bits - 1) / 2

    def dequantize(self, x, bits):  # utils/audio.py:254-255
        return 2 * x / (2**bits - 1) - 1

    def apply_inv_preemphasis(self, x):  # utils/audio.py:133-136
        if self.preemphasis == 0:
            raise RuntimeError(" !! Preemphasis is applied with factor 0.0. ")
        return scipy.signal.lfilter([1], [1, -self.preemphasis], x)

    def find_endpoint(self, wav, threshold_db=-40, min_silence_sec=0.8):  # utils/audio.py:203-210
        window_length = int(self.sample_rate * min_silence_sec)
        hop_length = int(window_length / 4)
        threshold = self._db_to_amp(threshold_db)
        for x in range(hop_length, len(wav) - window_length, hop_length):
            if np.max(wav[x:x + window_length]) < threshold:
                return x + hop_length
        return len(wav)

    def save_wav(self, wav, path):  # utils/audio.py:56-58
        wav_norm = np.asarray(wav) * (32767 / max(0.01, np.max(np.abs(wav))))
        scipy.io.wavfile.write(path, self.sample_rate, wav_norm.astype(np.int16))

    # ---------------------------------------------------------------- GPU Griffin-Lim
    def _handle(self):
        if self._gl is None:
            lib = _native.lib()
            cfg = _native.AudioConfig(
                n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                num_mels=self.num_mels, min_level_db=self.min_level_db, ref_level_db=self.ref_level_db,
                power=self.power, max_norm=self.max_norm, preemphasis=float(self.preemphasis),
                signal_norm=int(bool(self.signal_norm)), symmetric_norm=int(bool(self.symmetric_norm)),
                clip_norm=int(bool(self.clip_norm)))
            pinv = np.ascontiguousarray(np.linalg.pinv(self._build_mel_basis()), dtype=np.float64)
            h = ctypes.c_void_p()
            _native.check(lib.tts_gl_create(ctypes.byref(cfg), pinv.ctypes.data_as(ctypes.c_void_p),
                                            _native.stream_handle(), ctypes.byref(h)), "tts_gl_create")
            self._gl = (lib, h)
        return self._gl

    def __del__(self):
        try:
            if self._gl is not None:
                self._gl[0].tts_gl_destroy(self._gl[1])
        except Exception:
            pass

    def griffin_lim_batch(self, spec, frames, mode=_native.TTS_GL_FROM_MEL, phase_u=None, seed=0, iters=None):
        """spec: CUDA fp32 [B, Fmax, n] (frame-major); frames: list of F_b.  Returns CUDA fp64
        [B, hop*(Fmax-1)]; sentence b's waveform is the first hop*(F_b-1) samples."""
        lib, h = self._handle()
        iters = self.griffin_lim_iters if iters is None else iters
        spec = spec.float().contiguous()
        B, Fmax = spec.shape[0], spec.shape[1]
        wav = torch.zeros(B, self.hop_length * (Fmax - 1), dtype=torch.float64, device=spec.device)
        pu = None
        if phase_u is not None:
            pu = torch.as_tensor(phase_u, dtype=torch.float64).to(spec.device).contiguous()
        _native.check(lib.tts_gl_run(h, mode, ctypes.c_void_p(spec.data_ptr()), _native.i32_array(frames), B, Fmax,
                                     ctypes.c_void_p(pu.data_ptr()) if pu is not None else None, int(seed), int(iters),
                                     ctypes.c_void_p(wav.data_ptr()), _native.stream_handle()), "tts_gl_run")
        return wav

    # ---------------------------------------------------------------- numpy-stream phases (device)
    @contextlib.contextmanager
    def numpy_phases(self):
        """Within the block, every Griffin-Lim run on this processor's handle with no explicit
        phase_u (griffin_lim_batch, and the one-call tts_synth_run of a model using it) draws its
        initial phases from numpy's global generator ON THE DEVICE: bitwise np.random.rand(1025, F_b)
        per sentence in batch order (utils/audio.py:183), without the host draw or its upload
        (tts_gl_set_phase_state, phase_mt.hip).  On exit numpy's global state is where the same
        draws would have left it."""
        lib, h = self._handle()
        st = np.random.get_state()
        if st[0] != "MT19937":
            raise RuntimeError("numpy's global generator is not the legacy MT19937")
        key = np.ascontiguousarray(st[1], dtype=np.uint32)
        _native.check(lib.tts_gl_set_phase_state(h, key.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), int(st[2])),
                      "tts_gl_set_phase_state")
        try:
            yield self
            out = np.empty(624, np.uint32)
            pos = ctypes.c_int()
            _native.check(lib.tts_gl_get_phase_state(h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                     ctypes.byref(pos)), "tts_gl_get_phase_state")
            np.random.set_state(("MT19937", out, pos.value, st[3], st[4]))
        finally:
            lib.tts_gl_set_phase_state(h, None, 0)

    def draw_phases(self, frames, Fmax=None):
        """The initial phases numpy_phases() gives a batch of these frame counts, as a CUDA fp64
        [B, 1025, Fmax] tensor (advances the armed state; zero past each sentence's frames)."""
        lib, h = self._handle()
        Fmax = max(frames) if Fmax is None else Fmax
        out = torch.zeros(len(frames), self.n_fft // 2 + 1, Fmax, dtype=torch.float64, device="cuda")
        _native.check(lib.tts_gl_draw_phases(h, _native.i32_array(frames), len(frames), Fmax,
                                             ctypes.c_void_p(out.data_ptr()), _native.stream_handle()),
                      "tts_gl_draw_phases")
        return out

    def pcm16_join(self, wav, lens, gap=0, peak=None):
        """Synthesizer.tts's join + save_wav's conversion on the device (tts_gl_save_pcm16): the
        first lens[b] samples of each row of the CUDA fp64 [B, pitch] ``wav``, each followed by
        ``gap`` zeros, times 32767 / max(0.01, peak) truncated to int16 (peak None: max |y| of the
        request).  Returns the int16 samples as a numpy array, bytes equal to numpy's."""
        lib, h = self._handle()
        wav = wav if wav.dim() == 2 else wav.view(1, -1)
        assert wav.dtype == torch.float64 and wav.is_cuda and wav.stride(1) == 1
        n = np.ascontiguousarray([int(x) for x in lens], dtype=np.int64)
        total = int(n.sum()) + gap * len(n)
        out = torch.empty(max(total, 1), dtype=torch.int16, device=wav.device)
        _native.check(lib.tts_gl_save_pcm16(h, ctypes.c_void_p(wav.data_ptr()), wav.stride(0),
                                            n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(n), int(gap),
                                            -1.0 if peak is None else float(peak), ctypes.c_void_p(out.data_ptr()),
                                            _native.stream_handle()), "tts_gl_save_pcm16")
        return out[:total].cpu().numpy()

    def inv_mel_spectrogram_batch(self, mel, frames, seed=0, phase_u=None):
        return self.griffin_lim_batch(mel, frames, _native.TTS_GL_FROM_MEL, phase_u, seed)

    def last_gl_timing(self):
        lib, h = self._handle()
        ms, n = ctypes.c_float(), ctypes.c_int()
        lib.tts_gl_last_timing(h, ctypes.byref(ms), ctypes.byref(n))
        return dict(gl_loop_ms=ms.value, gl_iterations=n.value)

    def last_gl_path(self):
        """Iteration loop of the last run: "persistent", "fused" or "unfused" (tts_gl_last_path)."""
        lib, h = self._handle()
        p = ctypes.c_int()
        _native.check(lib.tts_gl_last_path(h, ctypes.byref(p)), "tts_gl_last_path")
        return _native.GL_PATHS[p.value]

    def profile_gl_kernels(self, reps=20):
        """Mean duration (ms) of the GL iteration and overlap-add kernels for the last batch."""
        lib, h = self._handle()
        n = len(_native.GL_KERNELS)
        ms = (ctypes.c_float * n)()
        _native.check(lib.tts_gl_profile(h, int(reps), ms, n), "tts_gl_profile")
        return dict(zip(_native.GL_KERNELS, [float(v) for v in ms]))

    # ---------------------------------------------------------------- analysis (device)
    def _set_mel_basis(self):
        lib, h = self._handle()
        if not self._mel_basis_set:
            basis = np.ascontiguousarray(self._build_mel_basis(), dtype=np.float64)
            _native.check(lib.tts_gl_set_mel_basis(h, basis.ctypes.data_as(ctypes.c_void_p)), "tts_gl_set_mel_basis")
            self._mel_basis_set = True
        return lib, h

    def _analyze(self, wav, N, want_linear, want_mel, Fmax=None):
        """tts_gl_analyze: one STFT per frame, either or both of the outputs (None where not asked), Fmax
        rows per sentence (None: the longest sentence's frames)."""
        lib, h = self._set_mel_basis() if want_mel else self._handle()
        wav = wav.to(torch.float64).contiguous()
        B, Nmax = wav.shape
        F = [1 + int(n) // self.hop_length for n in N]
        Fmax = max(F) if Fmax is None else int(Fmax)
        lin = torch.empty(B, Fmax, self.n_fft // 2 + 1, device=wav.device) if want_linear else None
        mel = torch.empty(B, Fmax, self.num_mels, device=wav.device) if want_mel else None
        _native.check(lib.tts_gl_analyze(h, ctypes.c_void_p(wav.data_ptr()), _native.i32_array(N), B, Nmax,
                                         ctypes.c_void_p(lin.data_ptr()) if want_linear else None,
                                         ctypes.c_void_p(mel.data_ptr()) if want_mel else None, Fmax,
                                         _native.stream_handle()), "tts_gl_analyze")
        return mel, lin, F

    def melspectrogram_batch(self, wav, N):
        """wav: CUDA float64 [B, Nmax]; N: samples per sentence.  Returns (CUDA float32
        [B, Fmax, num_mels] frame-major, frames per sentence = 1 + N // hop)."""
        lib, h = self._set_mel_basis()
        wav = wav.to(torch.float64).contiguous()
        B, Nmax = wav.shape
        F = [1 + int(n) // self.hop_length for n in N]
        mel = torch.empty(B, max(F), self.num_mels, device=wav.device)
        _native.check(lib.tts_gl_melspectrogram(h, ctypes.c_void_p(wav.data_ptr()), _native.i32_array(N), B, Nmax,
                                                ctypes.c_void_p(mel.data_ptr()), max(F), _native.stream_handle()),
                      "tts_gl_melspectrogram")
        return mel, F

    def spectrogram_batch(self, wav, N):
        """wav: CUDA float64 [B, Nmax]; N: samples per sentence.  Returns (CUDA float32
        [B, Fmax, num_freq] frame-major, the layout griffin_lim_batch(mode=TTS_GL_FROM_LINEAR) takes,
        frames per sentence)."""
        _, lin, F = self._analyze(wav, N, True, False)
        return lin, F

    def features_batch(self, wav, N, Fmax=None):
        """melspectrogram_batch and spectrogram_batch from one STFT per frame, as collate_fn needs them
        (datasets/TTSDataset.py:191-192).  Returns (mel, linear, frames per sentence).  Fmax: rows per
        sentence of both outputs (default: the longest sentence's frames); rows at and beyond a sentence's
        frames are zero, which is collate_fn's zero frame and padding."""
        return self._analyze(wav, N, True, True, Fmax)

    def melspectrogram(self, y):  # utils/audio.py:146-152 -> ndarray [num_mels, frames]
        self._handle()  # raises without a GPU / library: no CPU fallback
        y = np.asarray(y, dtype=np.float64)
        mel, F = self.melspectrogram_batch(torch.from_numpy(y).cuda()[None], [len(y)])
        return mel[0, :F[0]].T.double().cpu().numpy()

    def spectrogram(self, y):  # utils/audio.py:138-144 -> ndarray [num_freq, frames]
        self._handle()  # raises without a GPU / library: no CPU fallback
        y = np.asarray(y, dtype=np.float64)
        lin, F = self.spectrogram_batch(torch.from_numpy(y).cuda()[None], [len(y)])
        return lin[0, :F[0]].T.double().cpu().numpy()

    def out_linear_to_mel_batch(self, linear, frames):
        """linear: CUDA float32 [B, Fmax, num_freq] (frame-major: a Tacotron's out["linear"], or
        spectrogram_batch's output); frames: list of F_b.  Returns CUDA float32 [B, Fmax, num_mels],
        rows at and beyond F_b zero (tts_gl_linear_to_mel)."""
        lib, h = self._set_mel_basis()
        linear = linear.float().contiguous()
        B, Fmax = linear.shape[0], linear.shape[1]
        mel = torch.empty(B, Fmax, self.num_mels, device=linear.device)
        _native.check(lib.tts_gl_linear_to_mel(h, ctypes.c_void_p(linear.data_ptr()), _native.i32_array(frames), B,
                                               Fmax, ctypes.c_void_p(mel.data_ptr()), _native.stream_handle()),
                      "tts_gl_linear_to_mel")
        return mel

    def out_linear_to_mel(self, linear_spec):  # utils/audio.py:174-180 -> ndarray [num_mels, T]
        self._handle()  # raises without a GPU / library: no CPU fallback
        linear_spec = np.asarray(linear_spec, dtype=np.float32)
        T = linear_spec.shape[1]
        lin = torch.from_numpy(np.ascontiguousarray(linear_spec.T)).cuda()[None]
        return self.out_linear_to_mel_batch(lin, [T])[0].T.double().cpu().numpy()

    def trim_silence(self, wav):
        """utils/audio.py:212-217 on the host: drop 0.1 s margins, then librosa 0.6.2
        effects.trim(top_db=40, frame_length=1024, hop_length=256) restated (rms of centre-padded
        frames, power_to_db against the max, keep frames above -top_db)."""
        margin = int(self.sample_rate * 0.1)
        wav = wav[margin:-margin]
        frame_length, hop_length, top_db = 1024, 256, 40
        yp = np.pad(wav, frame_length // 2, mode="reflect")
        n_frames = 1 + (len(yp) - frame_length) // hop_length
        idx = np.arange(frame_length)[:, None] + hop_length * np.arange(n_frames)[None, :]
        mse = np.sqrt(np.mean(np.abs(yp[idx]) ** 2, axis=0)) ** 2
        db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
        nz = np.flatnonzero(db > -top_db)
        if nz.size == 0:
            return wav[0:0]
        return wav[int(nz[0]) * hop_length:min(len(wav), (int(nz[-1]) + 1) * hop_length)]

    @staticmethod
    def _read_wav(filename):
        """(sample rate, float64 samples) of a wav file: soundfile's conversion (PCM / 2**(bits-1))."""
        file_sr, x = scipy.io.wavfile.read(filename)
        if x.dtype == np.int16:
            x = x / 32768.0
        elif x.dtype == np.int32:
            x = x / 2147483648.0
        elif x.dtype == np.uint8:
            x = (x.astype(np.float64) - 128.0) / 128.0
        else:
            x = x.astype(np.float64)
        return file_sr, x

    @staticmethod
    def _to_mono_f32(x):
        """librosa.load's conversion of _read_wav's samples ([N] or [N, C]): float32, then to_mono's mean
        over the channels (float32 sum in channel order, divided by C)."""
        x = np.asarray(x, dtype=np.float32)
        if x.ndim == 1:
            return x
        acc = x[:, 0].copy()
        for c in range(1, x.shape[1]):
            acc = acc + x[:, c]
        return acc / np.float32(x.shape[1])

    def load_wav(self, filename, sr=None):
        """utils/audio.py:235-246.  Without ``sr``: soundfile's float64 conversion (PCM / 2**(bits-1)).
        With ``sr`` (utils/audio.py:239, librosa.load(filename, sr=sr)): float32 conversion, mono mix,
        resampling to ``sr`` on the device (resample_batch, a batch of one), and a float32 ndarray out.
        int16 files convert exactly; other sample widths are converted as _read_wav does and then rounded
        to float32 (audioread's own handling of those widths is not reproduced).  Trimming after a resample
        runs the float64 trim_silence on the float32-valued samples; librosa's float32 arithmetic inside
        effects.trim is not reproduced."""
        file_sr, x = self._read_wav(filename)
        if sr is not None:
            x = self._to_mono_f32(x)
            wav, n = self.resample_batch(torch.from_numpy(x.astype(np.float64)).cuda()[None], [len(x)], file_sr, sr)
            x = wav[0, :n[0]].cpu().numpy().astype(np.float32)
            if self.do_trim_silence:
                x = self.trim_silence(x.astype(np.float64)).astype(np.float32)
            assert self.sample_rate == sr, "%s vs %s" % (self.sample_rate, sr)
            return x
        if self.do_trim_silence:
            x = self.trim_silence(x)
        assert self.sample_rate == file_sr, "%s vs %s" % (self.sample_rate, file_sr)
        return x

    # ---------------------------------------------------------------- silence (device)
    TRIM_TOP_DB, TRIM_FRAME_LENGTH, TRIM_HOP_LENGTH = 40, 1024, 256  # utils/audio.py:216

    def _trim_margin(self):  # utils/audio.py:214
        return int(self.sample_rate * 0.1)

    def _trim_min_samples(self):
        """Shortest wav trim_silence_batch takes: the reflect padding of the margin-stripped signal by
        frame_length / 2 needs frame_length / 2 + 1 samples (np.pad raises ValueError below that)."""
        return 2 * self._trim_margin() + self.TRIM_FRAME_LENGTH // 2 + 1

    @staticmethod
    def _wav_batch(wav):
        assert wav.dim() == 2 and wav.dtype == torch.float64 and wav.is_cuda and wav.stride(1) == 1
        return wav

    def trim_silence_batch(self, wav, N):
        """trim_silence of every sentence of the CUDA float64 [B, Nmax] ``wav`` (N: samples per
        sentence) on the device (tts_gl_trim_silence).  Returns (start, end) as lists, relative to the
        margin-stripped signals: sentence b trimmed is wav[b, margin + start[b] : margin + end[b]].
        A sentence shorter than 2 * margin + 513 samples raises."""
        lib, h = self._handle()
        wav = self._wav_batch(wav)
        B = len(N)
        start, end = (ctypes.c_int32 * B)(), (ctypes.c_int32 * B)()
        _native.check(lib.tts_gl_trim_silence(h, ctypes.c_void_p(wav.data_ptr()), wav.stride(0), _native.i32_array(N),
                                              B, self._trim_margin(), self.TRIM_FRAME_LENGTH, self.TRIM_HOP_LENGTH,
                                              float(self.TRIM_TOP_DB), start, end, _native.stream_handle()),
                      "tts_gl_trim_silence")
        return list(start), list(end)

    def find_endpoint_batch(self, wav, N, threshold_db=-40, min_silence_sec=0.8):
        """find_endpoint of the first N[b] samples of every row of the CUDA float64 [B, Nmax] ``wav`` on
        the device (tts_gl_find_endpoint); window, hop and threshold as find_endpoint computes them.
        Returns the list of endpoints."""
        lib, h = self._handle()
        wav = self._wav_batch(wav)
        B = len(N)
        window_length = int(self.sample_rate * min_silence_sec)
        hop_length = int(window_length / 4)
        threshold = float(self._db_to_amp(threshold_db))
        end = (ctypes.c_int32 * B)()
        _native.check(lib.tts_gl_find_endpoint(h, ctypes.c_void_p(wav.data_ptr()), wav.stride(0), _native.i32_array(N),
                                               B, window_length, hop_length, threshold, end,
                                               _native.stream_handle()), "tts_gl_find_endpoint")
        return list(end)

    def take_segments(self, wav, start, lens):
        """wav[b, start[b] : start[b] + lens[b]] of a CUDA float64 [B, pitch] batch as a CUDA float64
        [B, max(lens)] batch, zeros behind each segment (tts_gl_take_segments)."""
        lib, h = self._handle()
        wav = self._wav_batch(wav)
        B = len(lens)
        out = torch.empty(B, max(1, max(int(n) for n in lens)), dtype=torch.float64, device=wav.device)
        _native.check(lib.tts_gl_take_segments(h, ctypes.c_void_p(wav.data_ptr()), wav.stride(0),
                                               _native.i32_array(start), _native.i32_array(lens), B,
                                               ctypes.c_void_p(out.data_ptr()), out.stride(0),
                                               _native.stream_handle()), "tts_gl_take_segments")
        return out[:, :max(int(n) for n in lens)]

    # ---------------------------------------------------------------- resampling (device)
    def _set_resample_filter(self, res_type):
        lib, h = self._handle()
        if isinstance(res_type, str) and self._resample_filter == res_type:
            return lib, h
        half_win, num_table = resample_filter(res_type) if isinstance(res_type, str) else res_type
        half_win = np.ascontiguousarray(half_win, dtype=np.float64)
        self._resample_filter = None
        _native.check(lib.tts_gl_set_resample_filter(h, half_win.ctypes.data_as(ctypes.c_void_p), len(half_win),
                                                     int(num_table)), "tts_gl_set_resample_filter")
        if isinstance(res_type, str):
            self._resample_filter = res_type
        return lib, h

    def resample_batch(self, wav, N, orig_sr, target_sr=None, res_type="kaiser_best"):
        """librosa 0.6.2 resample(y, orig_sr, target_sr, res_type, fix=True) of every sentence of the CUDA
        float64 [B, Nmax] ``wav`` (N: samples per sentence) on the device (tts_gl_resample): resampy's
        resample_f with a float32 accumulator, then fix_length.  orig_sr: one rate or one per sentence;
        target_sr: default the processor's rate; res_type: "kaiser_best" or a (half_win, num_table) pair.
        Samples are rounded to float32 on load and every result is a float32 value; a sentence already at
        target_sr passes through.  Returns (CUDA float64 [B, max n_fix], n_fix per sentence); samples at
        and beyond a sentence's n_res are zero."""
        lib, h = self._set_resample_filter(res_type)
        wav = self._wav_batch(wav)
        B = len(N)
        rates = [int(orig_sr)] * B if np.ndim(orig_sr) == 0 else [int(r) for r in orig_sr]
        assert len(rates) == B and wav.shape[0] == B
        target_sr = int(self.sample_rate if target_sr is None else target_sr)
        n_fix = [resample_lengths(int(n), r, target_sr)[1] for n, r in zip(N, rates)]
        out = torch.empty(B, max(n_fix), dtype=torch.float64, device=wav.device)
        n_out = (ctypes.c_int32 * B)()
        _native.check(lib.tts_gl_resample(h, ctypes.c_void_p(wav.data_ptr()), wav.stride(0), _native.i32_array(N),
                                          _native.i32_array(rates), target_sr, B, ctypes.c_void_p(out.data_ptr()),
                                          out.stride(0), n_out, _native.stream_handle()), "tts_gl_resample")
        assert list(n_out) == n_fix
        return out, n_fix

    def load_wav_batch(self, filenames, sr=None):
        """load_wav of every file, as one ragged batch on the device: the files are read and converted
        on the host as load_wav does, uploaded once, and with do_trim_silence trimmed on the device
        (trim_silence_batch, take_segments).  Returns (CUDA float64 [B, Nmax], samples per sentence),
        what features_batch / melspectrogram_batch take.  A file too short to trim is kept whole with
        the reference's message (utils/audio.py:240-244).  With ``sr`` the files may have any mix of
        rates and channel counts: each is converted as load_wav(filename, sr) converts it, the batch is
        resampled to ``sr`` on the device (resample_batch), then trimmed; every sample is a float32 value."""
        self._handle()  # raises without a GPU / library: no CPU fallback
        xs, rates = [], []
        for filename in filenames:
            file_sr, x = self._read_wav(filename)
            if sr is None:
                assert self.sample_rate == file_sr, "%s vs %s" % (self.sample_rate, file_sr)
            else:
                x = self._to_mono_f32(x)
            xs.append(x)
            rates.append(file_sr)
        N = [len(x) for x in xs]
        host = np.zeros((len(xs), max(N)), dtype=np.float64)
        for b, x in enumerate(xs):
            host[b, :N[b]] = x
        wav = torch.from_numpy(host).cuda()
        if sr is not None:
            wav, N = self.resample_batch(wav, N, rates, sr)
            assert self.sample_rate == sr, "%s vs %s" % (self.sample_rate, sr)
        if not self.do_trim_silence:
            return wav, N
        trim = [b for b in range(len(xs)) if N[b] >= self._trim_min_samples()]
        for b, filename in enumerate(filenames):
            if b not in trim:
                print(f' [!] File cannot be trimmed for silence - {filename}')
        start, lens = [0] * len(xs), list(N)
        if trim:
            rows = wav if len(trim) == len(xs) else wav[trim].contiguous()
            s, e = self.trim_silence_batch(rows, [N[b] for b in trim])
            margin = self._trim_margin()
            for i, b in enumerate(trim):
                start[b], lens[b] = margin + s[i], e[i] - s[i]
        return self.take_segments(wav, start, lens), lens

    def _single(self, spec_nT, mode):
        self._handle()  # raises without a GPU / library: no CPU fallback
        spec_nT = np.asarray(spec_nT, dtype=np.float32)
        T = spec_nT.shape[1]
        spec = torch.from_numpy(np.ascontiguousarray(spec_nT.T)).cuda()[None]
        # utils/audio.py:183: np.random.rand(1025, T) from numpy's global generator (unseeded unless
        # the caller seeds it), continued on the device
        with self.numpy_phases():
            wav = self.griffin_lim_batch(spec, [T], mode)
        return wav[0].cpu().numpy()

    def inv_mel_spectrogram(self, mel_spectrogram):  # utils/audio.py:164-172
        return self._single(mel_spectrogram, _native.TTS_GL_FROM_MEL)

    def inv_spectrogram(self, spectrogram):  # utils/audio.py:154-162
        return self._single(spectrogram, _native.TTS_GL_FROM_LINEAR)


def wav_bytes(ap: AudioProcessor, wav) -> _io.BytesIO:
    out = _io.BytesIO()
    ap.save_wav(np.asarray(wav), out)
    return out
