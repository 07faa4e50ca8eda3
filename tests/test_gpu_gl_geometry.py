"""GPU: Griffin-Lim (csrc/griffin_lim.hip, gl_handle.hip) and the analysis half (audio_analysis.hip) at
twelve STFT geometries (gl_geometry_util.GEOMETRIES) instead of the one every other module runs
(hop 275 / win 1102): the reference's four other configs, window / hop ratios of 2, 4, 5, 6 and 8, odd
window, odd hop, and the window that fills the FFT (woff 0).  Each sentence is held against the oracle
(anchored at these geometries by test_gl_geometry_cpu.py) at the project's own tolerances: 1e-6
relative RMS at zero iterations, WAV_RTOL = 1e-4 with iterations, 1e-5 * max(1, |ref|max) for the
analysis outputs.  The loop a run takes is derived from the restated host predicates, not measured.

Runs: SHORT frame counts on the default path and with TTS_RESIDENT=0; BATCHED (B * Fmax > 1024) with the
wave kernels, with TTS_GL_WAVE=0, and with TTS_GL_WAVE=0 TTS_GL_FUSED=1.  One result per (geometry, run,
iterations) and one oracle waveform per (geometry, frame count, iterations) are computed and shared.

Measured on an MI355X (profiles/gl_geometry.json; worst sentence over every run of a geometry):
zero iterations 1.4e-7 .. 2.3e-7 (bound 1e-6); three iterations 1.7e-7 .. 7.3e-7, the mel and the linear
path alike, and sixty iterations 8.6e-7 .. 1.2e-6 at the four reference configs and 200 / 900 (bound 1e-4); analysis
outputs 4.8e-8 (linear) and 3.4e-8 (mel) at most (bound 1e-5); every bitwise identity holds.  Loops: the
default SHORT run is persistent at 200 / 900, 275 / 1101 and 277 / 1102, fused at the geometries of
gl_geometry_util.LAST_PERSISTENT_F, unfused at ratios 6 and 8; every BATCHED run unfused, fused when forced.

Finding: where win = 2 k hop (800 / 200, 1000 / 250, 1100 / 275, 1200 / 300, 2048 / 512, 1024 / 512) the
overlap-add contributor relation is not symmetric from six frames up (four at 1024 / 512), which the
persistent loop's slot reuse rests on; the host checked sentences of up to three frames only, and the
first run of 1200 / 300 here ended in the loop's timed-out hand-off.  gl_persistent_path now checks every
frame count and such runs take the fused loop (test_persistent_refusal_boundary).
"""
import ctypes

import numpy as np
import pytest
import torch

import gl_geometry_util as G
from audio_analysis_util import oracle_spectrogram
from conftest import load_pkg, rel_rms
from encoder_util import _env
from oracle.griffin_lim_oracle import AudioOracle

pytestmark = pytest.mark.gpu
ZERO_RTOL = 1e-6  # test_gpu_batched.test_griffin_lim_wave_kernel_initial_istft_vs_oracle
WAV_RTOL = 1e-4   # test_gpu_batched.WAV_RTOL

# name: (batched frame counts?, environment)
RUNS = {
    "short": (False, {}),
    "short_nonresident": (False, {"TTS_RESIDENT": 0}),
    "batched_wave": (True, {}),
    "batched_block": (True, {"TTS_GL_WAVE": 0}),
    "batched_block_fused": (True, {"TTS_GL_WAVE": 0, "TTS_GL_FUSED": 1}),
}
FOUR_RUNS = [r for r in RUNS if r != "batched_block_fused"]
MEL, LINEAR = 0, 1  # TTS_GL_FROM_MEL, TTS_GL_FROM_LINEAR


def _tol(ref):
    return 1e-5 * max(1.0, float(np.abs(ref).max()))  # test_gpu_audio_analysis._tol


def _cfg(audio_cfg, name, **over):
    return G.audio_kwargs(audio_cfg, name, **over)


def _sentence(name, F, mode):
    """One sentence's seeded uniform(0, 1) spectrogram [F, n] float32 and phases [1025, F]: one seed per
    (geometry, F, mode), so every batch a sentence appears in shares its oracle waveform."""
    rng = np.random.Generator(np.random.PCG64(100000 * G.NAMES.index(name) + 10 * F + mode))
    n_in = 80 if mode == MEL else G.NB
    return rng.uniform(0, 1, size=(F, n_in)).astype(np.float32), rng.uniform(0, 1, size=(G.NB, F))


def _batch(name, Fs, mode):
    Fmax = max(Fs)
    spec = np.zeros((len(Fs), Fmax, 80 if mode == MEL else G.NB), np.float32)
    pu = np.zeros((len(Fs), G.NB, Fmax))
    for b, F in enumerate(Fs):
        spec[b, :F], pu[b, :, :F] = _sentence(name, F, mode)
    return spec, pu


_REF, _GPU, _HIP_ERROR = {}, {}, []


class _gpu_call:
    """A HIP error (status TTS_ERR_HIP) fails the test that met it, and every later test of this module
    without another launch.  The persistent loop's timed-out hand-off is a status of its own: the handle
    works again after it (test_gpu_gl_gather_forms.py), so only the test that met it fails."""

    def __enter__(self):
        if _HIP_ERROR:
            pytest.fail("not run: an earlier call ended in " + _HIP_ERROR[0])

    def __exit__(self, kind, err, tb):
        if kind is not None and issubclass(kind, RuntimeError) and ("status 2" in str(err) or "HIP error" in str(err)) \
                and "timed out" not in str(err):
            _HIP_ERROR.append(str(err))


def _ref(audio_cfg, name, F, iters, mode):
    key = (name, F, iters, mode)
    if key not in _REF:
        o = AudioOracle(**_cfg(audio_cfg, name))
        spec, pu = _sentence(name, F, mode)
        inv = o.inv_mel_spectrogram if mode == MEL else o.inv_spectrogram
        ref = inv(spec.T, pu, iters)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _run(audio_cfg, name, Fs, iters, mode, env):
    """griffin_lim_batch on a processor built inside ``env``: (waveform [B, Nmax] numpy, loop taken)."""
    spec, pu = _batch(name, Fs, mode)
    with _gpu_call(), _env(**env):
        ap = load_pkg("audio").AudioProcessor(**_cfg(audio_cfg, name, griffin_lim_iters=iters))
        hop, win = G.hop_win(name)
        assert (ap.hop_length, ap.win_length) == (hop, win)
        wav = ap.griffin_lim_batch(torch.from_numpy(spec).cuda(), Fs, mode=mode, phase_u=pu)
        path = ap.last_gl_path()
        wav = wav.cpu().numpy()
    return wav, path


def _measure(audio_cfg, name, run, iters, mode=MEL, Fs=None):
    """One cached result per (geometry, run, iterations, mode): per-sentence relative RMS against the
    oracle, the loop taken, and whether the padding is exactly zero and the samples finite."""
    key = (name, run, iters, mode, tuple(Fs) if Fs else None)
    if key not in _GPU:
        batched, env = RUNS[run]
        Fs_ = list(Fs) if Fs else G.frame_counts(name, batched)
        wav, path = _run(audio_cfg, name, Fs_, iters, mode, env)
        hop, _ = G.hop_win(name)
        rel, pad_zero = [], True
        for b, F in enumerate(Fs_):
            n = hop * (F - 1)
            rel.append(rel_rms(wav[b, :n], _ref(audio_cfg, name, F, iters, mode)))
            pad_zero = pad_zero and bool(np.all(wav[b, n:] == 0))
        print(f"{name} {run} iters={iters} mode={mode} Fs={Fs_}: {path}, worst {max(rel):.3e} "
              f"(F={Fs_[int(np.argmax(rel))]})")
        _GPU[key] = dict(Fs=Fs_, wav=wav, path=path, rel=rel, pad_zero=pad_zero, finite=bool(np.isfinite(wav).all()))
    return _GPU[key]


def _check(r, tol):
    assert r["finite"]
    for F, d in zip(r["Fs"], r["rel"]):
        assert d < tol, (F, d)
    assert r["pad_zero"]


# ---------------------------------------------------------------- a, b: every loop against the oracle
@pytest.mark.parametrize("run", FOUR_RUNS)
@pytest.mark.parametrize("name", G.NAMES)
def test_zero_iterations_vs_oracle(audio_cfg, name, run):
    """The initial iSTFT and the final overlap-add alone: 1e-6, padding exactly 0."""
    _check(_measure(audio_cfg, name, run, 0), ZERO_RTOL)


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("name", G.NAMES)
def test_three_iterations_vs_oracle(audio_cfg, name, run):
    _check(_measure(audio_cfg, name, run, 3), WAV_RTOL)


@pytest.mark.parametrize("name", G.NAMES)
def test_bitwise_identities(audio_cfg, name):
    """The persistent loop equals the TTS_RESIDENT=0 loop, and the unfused block loop equals the forced
    fused block loop, bit for bit (where a geometry has one loop only, the two runs are that loop twice)."""
    a, b = _measure(audio_cfg, name, "short", 3), _measure(audio_cfg, name, "short_nonresident", 3)
    assert torch.equal(torch.from_numpy(a["wav"]), torch.from_numpy(b["wav"]))
    a, b = _measure(audio_cfg, name, "batched_block", 3), _measure(audio_cfg, name, "batched_block_fused", 3)
    assert np.array_equal(a["wav"], b["wav"])


# ---------------------------------------------------------------- c: the loop each run takes
@pytest.mark.parametrize("name", G.NAMES)
def test_expected_paths(audio_cfg, name):
    paths = {(run, it): _measure(audio_cfg, name, run, it)["path"]
             for run in RUNS for it in (0, 3) if (run, it) != ("batched_block_fused", 0)}
    if name in G.UNFUSED_ONLY:  # ceil(win / hop) > OLA_MAX: gl_fused_path is false whatever the batch
        assert set(paths.values()) == {"unfused"}, paths
        return
    assert paths["short_nonresident", 0] == paths["short_nonresident", 3] == "fused"
    assert paths["short", 0] == "fused"  # (no iteration: nothing for the persistent loop to do)
    for run in ("batched_wave", "batched_block"):
        assert paths[run, 0] == paths[run, 3] == "unfused"
    assert paths["batched_block_fused", 3] == "fused"
    if name == "r45_fit":  # both host conditions hold at every F (gl_geometry_util.PERSISTENT; the others recorded)
        assert paths["short", 3] == "persistent"
    if name in G.LAST_PERSISTENT_F:  # Fmax 40 is beyond what the host lets the persistent loop take
        assert paths["short", 3] == "fused"


# ---------------------------------------------------------------- d: either side of the host's refusal
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", list(G.LAST_PERSISTENT_F))
def test_persistent_refusal_boundary(audio_cfg, name, side):
    """A ragged batch the persistent loop is eligible for, its longest sentence on either side of the last F
    gl_persistent_path accepts: the gather layout's fit (r45_big 6 | 7, full 3 | 4) or the contributor
    relation's symmetry (the reference configs 5 | 6, half 3 | 4: where win = 2 k hop an edge frame reads a
    frame that does not read it back, the loop's slot reuse is not safe, and 300 / 1200 timed out in a
    hand-off wait before the host refused it).  Persistent below, the fused loop above, both within
    tolerance (a timed-out hand-off would raise in griffin_lim_batch)."""
    Fmax = G.LAST_PERSISTENT_F[name] + side
    Fs = [Fmax, 2, Fmax - 1]
    r = _measure(audio_cfg, name, "short", 3, Fs=Fs)
    _check(r, WAV_RTOL)
    assert r["path"] == G.expected_path(name, Fs) == ("fused" if side else "persistent")
    z = _measure(audio_cfg, name, "short", 0, Fs=Fs)
    _check(z, ZERO_RTOL)


# ---------------------------------------------------------------- e: the metric's 60 iterations
@pytest.mark.parametrize("name", G.REFERENCE_CONFIGS + ["r45_fit"])
def test_sixty_iterations(audio_cfg, name):
    """The four reference configs (win = 4 hop: fused, the persistent loop is refused from six frames up) and
    200 / 900, which stays persistent."""
    Fs = [40, 2, 13]
    r = _measure(audio_cfg, name, "short", 60, Fs=Fs)
    _check(r, WAV_RTOL)
    assert r["path"] == G.expected_path(name, Fs, iters=60) == ("persistent" if name == "r45_fit" else "fused")


# ---------------------------------------------------------------- f: the linear path
@pytest.mark.parametrize("run", ["short", "batched_wave"])
@pytest.mark.parametrize("name", ["de16k", "full", "eighth"])
def test_linear_path_three_iterations(audio_cfg, name, run):
    _check(_measure(audio_cfg, name, run, 3, mode=LINEAR), WAV_RTOL)


# ---------------------------------------------------------------- g: the analysis half
def _analysis_batch(name):
    """Noise-plus-chirp sentences of k hop - 1, k hop, k hop + 1 (k = 20) and 1024 + hop / 2 + 1 samples,
    padded to a common length with non-zero garbage after each sentence's samples."""
    hop, _ = G.hop_win(name)
    N = [20 * hop - 1, 20 * hop, 20 * hop + 1, 1024 + hop // 2 + 1]
    xs = [G.chirp_noise(n, 1000 * G.NAMES.index(name) + b) for b, n in enumerate(N)]
    wav = np.full((len(N), max(N) + 50), 0.37)
    wav[:, ::3] = -0.81
    for b, x in enumerate(xs):
        wav[b, :N[b]] = x
    return xs, wav, N


def _measure_analysis(audio_cfg, name):
    key = ("analysis", name)
    if key not in _GPU:
        hop, _ = G.hop_win(name)
        c = _cfg(audio_cfg, name)
        xs, wav, N = _analysis_batch(name)
        o = AudioOracle(**c)
        with _gpu_call():
            ap = load_pkg("audio").AudioProcessor(**c)
            wav_d = torch.from_numpy(wav).cuda()
            mel, lin, F = ap.features_batch(wav_d, N)
            lin2, F2 = ap.spectrogram_batch(wav_d, N)
            mel2, F3 = ap.melspectrogram_batch(wav_d, N)
        out = dict(N=N, F=F, same_F=F2 == F and F3 == F, shapes=(tuple(lin.shape), tuple(mel.shape)),
                   bitwise=torch.equal(lin2, lin) and torch.equal(mel2, mel), lin_err=[], lin_tol=[], mel_err=[],
                   mel_tol=[], pad_zero=True)
        for b, x in enumerate(xs):
            rl, rm = oracle_spectrogram(o, x), o.melspectrogram(x)
            assert rl.shape == (G.NB, F[b]) and rm.shape == (80, F[b])
            out["lin_err"].append(float(np.abs(lin[b, :F[b]].T.double().cpu().numpy() - rl).max()))
            out["mel_err"].append(float(np.abs(mel[b, :F[b]].T.double().cpu().numpy() - rm).max()))
            out["lin_tol"].append(_tol(rl))
            out["mel_tol"].append(_tol(rm))
            out["pad_zero"] = out["pad_zero"] and not lin[b, F[b]:].any() and not mel[b, F[b]:].any()
        print(f"{name} analysis N={N} F={F}: linear max err {max(out['lin_err']):.3e}, mel max err "
              f"{max(out['mel_err']):.3e}, tol {min(out['lin_tol'] + out['mel_tol']):.3e}")
        _GPU[key] = out
    return _GPU[key]


@pytest.mark.parametrize("name", G.NAMES)
def test_analysis_vs_oracle(audio_cfg, name):
    hop, _ = G.hop_win(name)
    r = _measure_analysis(audio_cfg, name)
    assert r["F"] == [1 + n // hop for n in r["N"]] and r["same_F"]
    assert r["F"][:3] == [20, 21, 21] and 1024 < r["N"][3] < 1024 + hop
    assert r["shapes"] == ((4, 21, G.NB), (4, 21, 80))
    assert r["bitwise"]  # features_batch == spectrogram_batch + melspectrogram_batch
    assert r["pad_zero"]
    for b in range(4):
        assert r["lin_err"][b] <= r["lin_tol"][b], b
        assert r["mel_err"][b] <= r["mel_tol"][b], b


# ---------------------------------------------------------------- h: analysis feeds synthesis
@pytest.mark.parametrize("name", ["de16k", "libri24k"])
def test_spectrogram_feeds_griffin_lim(audio_cfg, name):
    """As test_gpu_audio_analysis.test_gpu_spectrogram_feeds_griffin_lim: spectrogram_batch's device tensor
    through TTS_GL_FROM_LINEAR against inv_spectrogram(spectrogram(x)) through the host, phases from
    numpy's stream in both."""
    native = load_pkg("_native")
    ap = load_pkg("audio").AudioProcessor(**_cfg(audio_cfg, name, griffin_lim_iters=5))
    x = G.chirp_noise(20 * ap.hop_length + 7, 77)
    with _gpu_call():
        np.random.seed(4321)
        lin, F = ap.spectrogram_batch(torch.from_numpy(x).cuda()[None], [len(x)])
        with ap.numpy_phases():
            wav_dev = ap.griffin_lim_batch(lin, F, mode=native.TTS_GL_FROM_LINEAR)
        np.random.seed(4321)
        wav_host = ap.inv_spectrogram(ap.spectrogram(x))
    wav_dev = wav_dev[0, :ap.hop_length * (F[0] - 1)].cpu().numpy()
    assert wav_dev.shape == wav_host.shape and np.abs(wav_host).max() > 1e-3
    assert rel_rms(wav_dev, wav_host) < WAV_RTOL
    # ... and against the oracle on the same spectrogram and phases
    np.random.seed(4321)
    ref = AudioOracle(**_cfg(audio_cfg, name, griffin_lim_iters=5)).inv_spectrogram(lin[0, :F[0]].T.cpu().numpy())
    assert rel_rms(wav_dev, ref) < WAV_RTOL


# ---------------------------------------------------------------- i: tts_gl_create's argument checks
INVALID, UNSUPPORTED = 1, 3  # TTS_ERR_INVALID, TTS_ERR_UNSUPPORTED (include/tts_hip.h)


@pytest.mark.parametrize("over,status,message", [
    (dict(n_fft=1024), UNSUPPORTED, "n_fft"),
    (dict(win_length=1, hop_length=1), INVALID, "win_length"),
    (dict(win_length=2049), INVALID, "win_length"),
    (dict(hop_length=0), UNSUPPORTED, "hop_length"),
    (dict(hop_length=801), UNSUPPORTED, "hop_length"),  # win_length + 1
    (dict(num_mels=81), UNSUPPORTED, "num_mels"),
])
def test_create_argument_checks(over, status, message):
    native = load_pkg("_native")
    lib = native.lib()
    base = dict(n_fft=2048, hop_length=200, win_length=800, num_mels=80, min_level_db=-100.0, ref_level_db=20.0,
                power=1.5, max_norm=1.0, preemphasis=0.98, signal_norm=1, symmetric_norm=0, clip_norm=1)
    h = ctypes.c_void_p()
    cfg = native.AudioConfig(**{**base, **over})
    assert lib.tts_gl_create(ctypes.byref(cfg), None, native.stream_handle(), ctypes.byref(h)) == status
    assert h.value is None
    assert message in lib.tts_last_error().decode()
    # the same call with the valid arguments succeeds
    cfg = native.AudioConfig(**base)
    assert lib.tts_gl_create(ctypes.byref(cfg), None, native.stream_handle(), ctypes.byref(h)) == 0
    assert h.value
    lib.tts_gl_destroy(h)
