"""The device half of AudioProcessor's analysis calls against the reference's own outputs
(audio_analysis*.npz, tests/golden/make_golden_audio_analysis.py): spectrogram (tts_gl_analyze),
out_linear_to_mel (tts_gl_linear_to_mel), the fused features_batch on a ragged batch, the layout
contract with Griffin-Lim's TTS_GL_FROM_LINEAR input, and the argument checks of the two entry points.
Every case is a few dozen frames.
"""
import ctypes

import numpy as np
import pytest
import torch

from audio_analysis_util import EXCERPTS, Z, cfg, oracle_spectrogram
from conftest import load_pkg, rel_rms
from oracle.griffin_lim_oracle import AudioOracle

pytestmark = pytest.mark.gpu
WAV_RTOL = 1e-4  # the project's waveform tolerance (tests/test_audio_example.py)


def _tol(ref):
    return 1e-5 * max(1.0, float(np.abs(ref).max()))  # _mel_tol of tests/test_audio_example.py: float32 output


def _ap(i, **over):
    return load_pkg("audio").AudioProcessor(**cfg(i, **over))


def _ragged():
    """[xa, xb] padded to a common Nmax with non-zero garbage after each sentence's samples."""
    xs = [Z["xa"], Z["xb"]]
    N = [len(x) for x in xs]
    wav = np.full((2, max(N) + 50), 0.37)
    wav[:, ::3] = -0.81
    for b, x in enumerate(xs):
        wav[b, :N[b]] = x
    return torch.from_numpy(wav).cuda(), N


@pytest.mark.parametrize("e", EXCERPTS)
@pytest.mark.parametrize("i", range(10))
def test_gpu_spectrogram(i, e):
    ref = Z[f"lin{i}{e}"]
    lin = _ap(i).spectrogram(Z["x" + e])
    assert lin.shape == ref.shape
    err = np.abs(lin - ref).max()
    print(f"spectrogram setting {i} x{e}: max err {err:.3e} tol {_tol(ref):.3e}")
    assert err <= _tol(ref)


@pytest.mark.parametrize("e", EXCERPTS)
@pytest.mark.parametrize("i", range(10))
def test_gpu_out_linear_to_mel(i, e):
    ref = Z[f"l2m{i}{e}"]
    mel = _ap(i).out_linear_to_mel(Z[f"lin{i}{e}"].astype(np.float32))
    assert mel.shape == ref.shape
    err = np.abs(mel - ref).max()
    print(f"out_linear_to_mel setting {i} x{e}: max err {err:.3e} tol {_tol(ref):.3e}")
    assert err <= _tol(ref)


@pytest.mark.parametrize("i", [0, 9])
def test_gpu_features_batch_ragged(i):
    ap = _ap(i)
    wav, N = _ragged()
    mel, lin, F = ap.features_batch(wav, N)
    assert F == [21, 5] and lin.shape == (2, 21, 1025) and mel.shape == (2, 21, 80)
    assert lin.dtype == mel.dtype == torch.float32 and lin.is_cuda and mel.is_cuda
    for b, e in enumerate(EXCERPTS):
        x = torch.from_numpy(Z["x" + e]).cuda()[None]
        lin1, F1 = ap.spectrogram_batch(x, [N[b]])
        mel1, _ = ap.melspectrogram_batch(x, [N[b]])
        assert F1 == [F[b]]
        assert torch.equal(lin[b, :F[b]], lin1[0]) and torch.equal(mel[b, :F[b]], mel1[0])
        assert not lin[b, F[b]:].any() and not mel[b, F[b]:].any()
        assert np.abs(lin[b, :F[b]].T.double().cpu().numpy() - Z[f"lin{i}{e}"]).max() <= _tol(Z[f"lin{i}{e}"])
        assert np.abs(mel[b, :F[b]].T.double().cpu().numpy() - Z[f"mel{i}{e}"]).max() <= _tol(Z[f"mel{i}{e}"])
    lin2, F2 = ap.spectrogram_batch(wav, N)
    mel2, F3 = ap.melspectrogram_batch(wav, N)
    assert F2 == F and F3 == F
    assert torch.equal(lin2, lin) and torch.equal(mel2, mel)


def test_gpu_spectrogram_without_preemphasis():
    c = cfg(4, preemphasis=0.0)
    ref = oracle_spectrogram(AudioOracle(**c), Z["xa"])
    lin = load_pkg("audio").AudioProcessor(**c).spectrogram(Z["xa"])
    assert lin.shape == ref.shape
    assert np.abs(lin - ref).max() <= _tol(ref)
    assert np.abs(ref - Z["lin4a"]).max() > 100 * _tol(ref)  # (the FIR is not a no-op on this excerpt)


def test_gpu_spectrogram_feeds_griffin_lim():
    """spectrogram_batch's device tensor is TTS_GL_FROM_LINEAR's input as it stands: the same waveform
    as inv_spectrogram(spectrogram(x)) through the host, phases from numpy's stream in both."""
    native = load_pkg("_native")
    ap = _ap(6, griffin_lim_iters=5)
    xa = Z["xa"]
    np.random.seed(4321)
    lin, F = ap.spectrogram_batch(torch.from_numpy(xa).cuda()[None], [len(xa)])
    with ap.numpy_phases():
        wav_dev = ap.griffin_lim_batch(lin, F, mode=native.TTS_GL_FROM_LINEAR)
    np.random.seed(4321)
    wav_host = ap.inv_spectrogram(ap.spectrogram(xa))
    wav_dev = wav_dev[0, :ap.hop_length * (F[0] - 1)].cpu().numpy()
    assert wav_dev.shape == wav_host.shape and np.abs(wav_host).max() > 1e-3
    assert rel_rms(wav_dev, wav_host) < WAV_RTOL


@pytest.mark.parametrize("i", [3, 7])
def test_gpu_out_linear_to_mel_batch_padding(i):
    """[B, Fmax, 1025] with frames < Fmax: rows at and beyond a sentence's frames come back zero, whatever
    the input holds there, across whole and partial tiles of frames."""
    ap = _ap(i)
    frames, Fmax = [21, 5], 27
    lin = torch.full((2, Fmax, 1025), 0.25, device="cuda")
    for b, e in enumerate(EXCERPTS):
        lin[b, :frames[b]] = torch.from_numpy(Z[f"lin{i}{e}"].astype(np.float32).T).cuda()
    mel = ap.out_linear_to_mel_batch(lin, frames)
    assert mel.shape == (2, Fmax, 80) and mel.dtype == torch.float32 and mel.is_cuda
    for b, e in enumerate(EXCERPTS):
        ref = Z[f"l2m{i}{e}"]
        assert np.abs(mel[b, :frames[b]].T.double().cpu().numpy() - ref).max() <= _tol(ref)
        assert not mel[b, frames[b]:].any()


def test_gpu_argument_checks():
    native = load_pkg("_native")
    ap = _ap(1)
    lib, h = ap._handle()
    hop, s = ap.hop_length, native.stream_handle()
    wav = torch.zeros(1, 4 * hop, dtype=torch.float64, device="cuda")
    lin = torch.full((1, 5, 1025), 7.0, device="cuda")
    mel = torch.full((1, 5, 80), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def analyze(N, linear, mel_, Fmax):
        native.check(lib.tts_gl_analyze(h, p(wav), native.i32_array([N]), 1, wav.shape[1], linear, mel_, Fmax, s),
                     "tts_gl_analyze")

    def convert(F, Fmax):
        native.check(lib.tts_gl_linear_to_mel(h, p(lin), native.i32_array([F]), 1, Fmax, p(mel), s),
                     "tts_gl_linear_to_mel")

    with pytest.raises(RuntimeError, match="basis"):  # no mel basis on this handle yet
        convert(5, 5)
    with pytest.raises(RuntimeError, match="basis"):
        analyze(4 * hop, None, p(mel), 5)
    ap._set_mel_basis()
    with pytest.raises(RuntimeError, match="N\\[b\\]"):
        analyze(1, p(lin), None, 5)
    with pytest.raises(RuntimeError, match="N\\[b\\]"):
        analyze(4 * hop + 1, p(lin), None, 5)  # > Nmax
    with pytest.raises(RuntimeError, match="Fmax"):
        analyze(4 * hop, p(lin), None, 4)  # 1 + N / hop = 5 frames
    with pytest.raises(RuntimeError, match="output"):
        analyze(4 * hop, None, None, 5)
    with pytest.raises(RuntimeError, match="F\\[b\\]"):
        convert(0, 5)
    with pytest.raises(RuntimeError, match="F\\[b\\]"):
        convert(6, 5)
    torch.cuda.synchronize()
    assert bool((lin == 7.0).all()) and bool((mel == 7.0).all())  # nothing was launched
    analyze(4 * hop, p(lin), p(mel), 5)  # the same arguments, valid
    convert(5, 5)
    torch.cuda.synchronize()
    assert not bool((lin == 7.0).any()) and not bool((mel == 7.0).any())
