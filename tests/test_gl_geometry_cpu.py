"""CPU: the ground the GPU geometry tests (test_gpu_gl_geometry.py) stand on.

- The table of gl_geometry_util.py gives the hop / win / woff it says, through the oracle's own
  ``int(ms / 1000.0 * sr)``.
- The oracle's fixtures from the reference exist at 275 / 1102 only, so at every geometry its stft and
  istft are held against a second restatement built from the definition (explicit window, np.fft.rfft /
  irfft per frame, per-frame overlap-add loops): measured here bitwise equal for both (scipy.fftpack and
  np.fft share one FFT); asserted within 1 ulp of complex64 for the STFT and 1e-6 relative RMS for the iSTFT.
- The tests' power to discriminate, on the oracle alone.  (A) the window truncated to its first 4 hop
  samples (a sample's fifth overlap-add contributor lost) moves the waveform by 8.6e-3 .. 4.1e-2 (0
  iterations) and 2.0e-2 .. 1.5e-1 (3 iterations) at 200 / 900 and 256 / 1152, but by <= 5.3e-6 at the
  default 275 / 1102, below WAV_RTOL: only the new geometries see it.  (B) the padded window rolled by
  one sample moves the zero-iteration waveform by 1.5e-3 .. 5.1e-3 at every geometry.
- The restated loop predicates agree with what the GPU tests assume of each geometry: where win = 2 k hop
  (the reference's four other configs among them) the overlap-add contributor relation stops being
  symmetric at six frames, so the persistent loop must be refused from there on.
"""
import numpy as np
import pytest

import gl_geometry_util as G
from conftest import rel_rms
from oracle.griffin_lim_oracle import AudioOracle, istft, stft

WAV_RTOL = 1e-4   # the GPU tests' waveform tolerance with iterations
ZERO_RTOL = 1e-6  # ... and at zero iterations


def _oracle(audio_cfg, name=None, **over):
    return AudioOracle(**(G.audio_kwargs(audio_cfg, name, **over) if name else {**audio_cfg, **over}))


@pytest.mark.parametrize("name", G.NAMES)
def test_table_geometry(audio_cfg, name):
    hop, win = G.hop_win(name)
    o = _oracle(audio_cfg, name)
    assert (o.n_fft, o.hop_length, o.win_length) == (G.NFFT, hop, win)
    assert o.mel_fmax <= o.sample_rate / 2
    woff = (2048 - win) // 2
    assert G._geo(hop, win)[0] == woff
    expect = {"de16k": 624, "best20k": 524, "kusal22k": 474, "libri24k": 424, "r45_fit": 574, "r45_big": 448,
              "oddwin": 473, "oddhop": 473, "full": 0, "half": 512, "sixth": 424, "eighth": 512}
    assert woff == expect[name]
    assert 1 <= hop < win <= 2048  # (hop == win is left out: the sum-square vanishes at the frame joins)


def test_table_derived_quantities():
    assert G._geo(200, 800) == (624, 624, 800)    # winp == win
    assert G._geo(275, 1101) == (473, 472, 1104)  # odd win: fb = woff - 1
    assert G._geo(512, 2048) == (0, 0, 2048)
    for hop in (256, 512):  # the scan chunk edges
        assert [hop * (F - 1) for F in G.SCAN_EDGE[hop]] == [4096, 8192]
    assert len(G.BATCHED) * max(G.BATCHED) > 1024 >= len(G.SHORT) * max(G.SHORT)


@pytest.mark.parametrize("name", G.NAMES)
def test_oracle_stft_vs_definition(name):
    """Within 1 ulp of complex64 (of the larger component); measured bitwise equal."""
    hop, win = G.hop_win(name)
    for F in (2, 3, 5, 12, 40):
        x = G.chirp_noise(hop * (F - 1), 7 + F)
        a, b = stft(x, G.NFFT, hop, win), G.direct_stft(x, hop, win)
        assert a.dtype == b.dtype == np.complex64 and a.shape == b.shape == (G.NB, F)
        ulp = np.spacing(np.maximum(np.abs(b.real), np.abs(b.imag)))
        assert (np.abs(a.real - b.real) <= ulp).all() and (np.abs(a.imag - b.imag) <= ulp).all(), F


@pytest.mark.parametrize("name", G.NAMES)
def test_oracle_istft_vs_definition(audio_cfg, name):
    """1e-6 relative RMS; measured 0 (bitwise equal) at every geometry and frame count."""
    hop, win = G.hop_win(name)
    o = _oracle(audio_cfg, name)
    for F in (2, 3, 5, 12, 40):
        spec, pu = G.gl_inputs([F], 100 + F)
        S = o.mel_magnitude(spec[0].T) * np.exp(2j * np.pi * pu[0])
        a, b = istft(S, hop, win), G.direct_istft(S, hop, win)
        assert a.shape == b.shape == (hop * (F - 1),) and np.abs(b).max() > 0
        d = rel_rms(a, b)
        print(f"{name} F={F}: oracle istft vs definition {d:.3e}")
        assert d < 1e-6, F


def _moved(o, hop, kind, F, iters):
    spec, pu = G.gl_inputs([F], 600 + F)  # (seed base 300 gave 7.2e-3 at 256 / 1152, F = 5, 3 iterations)
    ref = o.inv_mel_spectrogram(spec[0].T, pu[0], iters)
    with G.mistake(kind, hop):
        bad = o.inv_mel_spectrogram(spec[0].T, pu[0], iters)
    again = o.inv_mel_spectrogram(spec[0].T, pu[0], iters)
    assert np.array_equal(ref, again)  # (the mistake is gone with its block)
    return rel_rms(bad, ref)


@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("name", ["r45_fit", "r45_big"])
def test_truncated_window_is_seen_at_ratio_above_four(audio_cfg, name, iters):
    """(A) at 200 / 900 and 256 / 1152: more than 100 x the GPU tolerance of the same iteration count."""
    hop, _ = G.hop_win(name)
    o = _oracle(audio_cfg, name)
    tol = ZERO_RTOL if iters == 0 else WAV_RTOL
    for F in (3, 5, 12, 40):
        d = _moved(o, hop, "truncate", F, iters)
        print(f"{name} F={F} iters={iters}: truncated window moves the waveform by {d:.3e}")
        assert d > 100 * tol, F


@pytest.mark.parametrize("iters", [0, 3])
def test_truncated_window_is_not_seen_at_default_geometry(audio_cfg, iters):
    """(A) at 275 / 1102, the one geometry the suite ran before: below WAV_RTOL (measured <= 5.3e-6), which is
    why the other geometries are needed."""
    o = _oracle(audio_cfg)
    assert (o.hop_length, o.win_length) == (275, 1102)
    for F in (3, 5, 12, 40):
        d = _moved(o, 275, "truncate", F, iters)
        print(f"275/1102 F={F} iters={iters}: truncated window moves the waveform by {d:.3e}")
        assert d < WAV_RTOL, F


@pytest.mark.parametrize("name", G.NAMES)
def test_rolled_window_is_seen_everywhere(audio_cfg, name):
    """(B) at zero iterations: more than 1e-3 at every geometry (1000 x the GPU tolerance there)."""
    hop, _ = G.hop_win(name)
    o = _oracle(audio_cfg, name)
    for F in (5, 40):
        d = _moved(o, hop, "roll", F, 0)
        print(f"{name} F={F}: rolled window moves the waveform by {d:.3e}")
        assert d > 1e-3, F


def test_restated_predicates():
    """What the GPU module assumes of each geometry, from the restated host predicates."""
    last = {}
    for name in G.NAMES:
        hop, win = G.hop_win(name)
        assert G.fused_geometry(hop, win) == (name not in G.UNFUSED_ONLY)
        if name not in G.UNFUSED_ONLY:
            last[name] = next((F - 1 for F in range(2, 45) if not G.persistent_geometry(hop, win, F)), None)
    assert {n for n, F in last.items() if F is None} == set(G.PERSISTENT)
    assert {n: F for n, F in last.items() if F is not None} == G.LAST_PERSISTENT_F
    # which of the two conditions ends it: the relation's symmetry (win = 2 k hop) or the gather layout
    for name in G.REFERENCE_CONFIGS + ["full", "half"]:
        hop, win = G.hop_win(name)
        assert not any(G.contrib_symmetric(hop, win, F) for F in range(6, 45)), name
    for name, Fok in (("r45_big", 6), ("full", 3)):
        hop, win = G.hop_win(name)
        assert G.gather_fits(hop, win, Fok) and not G.gather_fits(hop, win, Fok + 1)
    assert all(G.gather_fits(*G.hop_win(n), F) for n in G.REFERENCE_CONFIGS for F in range(2, 45))
    # the default geometry, which every other module runs, keeps the persistent loop at every length
    assert all(G.contrib_symmetric(275, 1102, F) and G.gather_fits(275, 1102, F) for F in range(2, 45))
    assert G.expected_path("sixth", G.SHORT, forced_fused=True) == "unfused"
    assert G.expected_path("r45_fit", G.SHORT) == "persistent"
    assert G.expected_path("r45_fit", G.SHORT, iters=0) == "fused"
    assert G.expected_path("r45_fit", G.SHORT, resident=False) == "fused"
    assert G.expected_path("r45_fit", G.BATCHED) == "unfused"
    assert G.expected_path("r45_fit", G.BATCHED, forced_fused=True) == "fused"
    assert G.expected_path("de16k", G.SHORT) == "fused" and G.expected_path("de16k", [5, 2, 3]) == "persistent"
