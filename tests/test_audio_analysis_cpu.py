"""The analysis half of the reference AudioProcessor (utils/audio.py:60-66, :79-94, :121-152, :174-180,
:219-255) on two excerpts of tests/inputs/example_1.wav, replayed on the reference's own class by
tests/golden/make_golden_audio_analysis.py (audio_analysis*.npz; librosa 0.6.2 restated, its internals
unpinned).  Here, without a GPU: the fixture against the oracle restatement, and the package's host
helpers against the fixture.  tests/test_gpu_audio_analysis.py holds the device half.
"""
import numpy as np
import pytest

from audio_analysis_util import EXCERPTS, SETTINGS, Z, cfg, oracle_out_linear_to_mel, oracle_spectrogram
from conftest import load_pkg
from oracle.griffin_lim_oracle import AudioOracle


def _close(got, ref, rtol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.abs(got - ref).max() <= rtol * max(1.0, float(np.abs(ref).max()))


def _ap(i=0, **over):
    return load_pkg("audio").AudioProcessor(**cfg(i, **over))


def test_fixture_shapes():
    assert len(SETTINGS) == 10
    hop = AudioOracle(**cfg(0)).hop_length
    for e, frames in zip(EXCERPTS, (21, 5)):
        x = Z["x" + e]
        assert x.dtype == np.float64 and len(x) % hop != 0 and 1 + len(x) // hop == frames
        for i in range(10):
            assert Z[f"lin{i}{e}"].shape == (1025, frames) and Z[f"lin{i}{e}"].dtype == np.float64
            assert Z[f"mel{i}{e}"].shape == Z[f"l2m{i}{e}"].shape == (80, frames)
    assert len(Z["xb"]) < 1024 + hop  # every frame of xb reaches the reflect padding


@pytest.mark.parametrize("e", EXCERPTS)
@pytest.mark.parametrize("i", range(10))
def test_oracle_spectrogram_matches_reference(i, e):
    _close(oracle_spectrogram(AudioOracle(**cfg(i)), Z["x" + e]), Z[f"lin{i}{e}"], 1e-9)


@pytest.mark.parametrize("e", EXCERPTS)
@pytest.mark.parametrize("i", range(10))
def test_oracle_out_linear_to_mel_matches_reference(i, e):
    lin32 = Z[f"lin{i}{e}"].astype(np.float32)
    _close(oracle_out_linear_to_mel(AudioOracle(**cfg(i)), lin32), Z[f"l2m{i}{e}"], 1e-9)


@pytest.mark.parametrize("i", range(10))
def test_normalize(i):
    _close(_ap(i)._normalize(Z["norm_in"]), Z[f"norm{i}"], 1e-12)


def test_amp_to_db():
    _close(_ap()._amp_to_db(Z["amp_in"]), Z["amp_to_db"], 1e-12)


def test_apply_preemphasis():
    _close(_ap().apply_preemphasis(Z["xa"][:1000]), Z["preemph"], 1e-12)
    with pytest.raises(RuntimeError):
        _ap(preemphasis=0.0).apply_preemphasis(Z["xa"][:1000])


@pytest.mark.parametrize("qc", [8, 10])
def test_mulaw(qc):
    AP = load_pkg("audio").AudioProcessor
    enc = AP.mulaw_encode(Z["xa"][:1000], qc)  # a staticmethod, as in the reference
    assert enc.dtype == Z[f"mulaw_enc{qc}"].dtype and np.array_equal(enc, Z[f"mulaw_enc{qc}"])
    _close(AP.mulaw_decode(2 * enc / (2 ** qc - 1) - 1, qc), Z[f"mulaw_dec{qc}"], 1e-12)


def test_quantize_dequantize_encode_16bits():
    ap, x = _ap(), Z["xa"][:1000]
    q = ap.quantize(x, 8)
    _close(q, Z["quantize8"], 1e-12)
    _close(ap.dequantize(q, 8), Z["dequantize8"], 1e-12)
    pcm = ap.encode_16bits(x * 8.0)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, Z["encode_16bits"])


def test_linear_to_mel_mel_to_linear():
    ap = _ap()
    mel = ap._linear_to_mel(Z["frame_mag"])
    _close(mel, Z["linear_to_mel"], 1e-12)
    _close(ap._mel_to_linear(mel), Z["mel_to_linear"], 1e-12)
