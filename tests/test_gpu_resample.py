"""GPU: resampling on the device (tts_gl_set_resample_filter, tts_gl_resample; AudioProcessor.resample_batch,
load_wav(sr=...), load_wav_batch(sr=...)) against resample_util's numpy restatement of librosa 0.6.2 load /
resample and resampy 0.2.x resample_f.  The kernel performs the restatement's operations in its order, so
every comparison is bitwise equality of the n_fix float32 samples: no tolerance is owed."""
import ctypes
import functools
import re

import numpy as np
import pytest
import scipy.io.wavfile
import torch

import resample_util as ru
import silence_util as su
from conftest import load_pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _case(orig, target, N, small=False):
    """(signal, restatement) of one case, computed once."""
    x = ru.signal(N, orig)
    y = ru.resample_ref(x, orig, target, ru.small_filter() if small else None)
    y.setflags(write=False)
    x.setflags(write=False)
    return x, y


def _ragged(rows, pitch=None, fill=0.0):
    N = [len(r) for r in rows]
    host = np.full((len(rows), max(N) if pitch is None else pitch), fill, dtype=np.float64)
    for b, r in enumerate(rows):
        host[b, :N[b]] = r
    return torch.from_numpy(host).cuda(), N


def _same(got, want):
    return got.shape == want.shape and np.array_equal(ru.bits(got), ru.bits(want))


def _check_rows(out, n_fix, wants):
    assert out.dtype == torch.float64 and out.shape == (len(wants), max(len(w) for w in wants))
    assert n_fix == [len(w) for w in wants]
    host = out.cpu().numpy()
    for b, w in enumerate(wants):
        got = host[b, :n_fix[b]]
        assert np.array_equal(got, got.astype(np.float32)), b  # every value is a float32
        bad = int((ru.bits(got) != ru.bits(w)).sum())
        print(f"sentence {b}: {n_fix[b]} samples, {bad} differ from the restatement")
        assert bad == 0, b
        assert not host[b, n_fix[b]:].any(), b


def _raw(ap, src, N, rates, target, dst, n_out=None, B=None):
    """tts_gl_resample itself: (status, error text, n_out)."""
    lib, h = ap._handle()
    native = load_pkg("_native")
    B = len(N) if B is None else B
    n_out = (ctypes.c_int32 * max(1, len(N)))() if n_out is None else n_out
    st = lib.tts_gl_resample(h, ctypes.c_void_p(src.data_ptr()) if src is not None else None,
                             src.stride(0) if src is not None else 0, native.i32_array(N), native.i32_array(rates),
                             target, B, ctypes.c_void_p(dst.data_ptr()) if dst is not None else None,
                             dst.stride(0) if dst is not None else 0, n_out, native.stream_handle())
    return st, lib.tts_last_error().decode(), list(n_out)


def test_ragged_batch_of_mixed_rates():
    ap = su.processor()
    assert ap.sample_rate == 22050
    cases = [c for c in ru.CASES if c[1] == 22050]
    assert len(cases) == 9 and len(ru.CASES) == 10
    rows = [_case(*c) for c in cases]
    wav, N = _ragged([x for x, _ in rows])
    out, n_fix = ap.resample_batch(wav, N, [c[0] for c in cases])
    _check_rows(out, n_fix, [y for _, y in rows])
    assert n_fix[2] == 2 and out[2, 1] == 0 and out[2, 0] != 0  # one output plus one padding zero
    assert torch.equal(out[8, :600].float().cpu(), torch.from_numpy(rows[8][0].copy()))  # the pass-through
    # the same again, from the cached registers
    again, _ = ap.resample_batch(wav, N, [c[0] for c in cases])
    assert torch.equal(again, out)
    # one rate for the whole batch, and a sentence alone, give the same bits
    alone, n1 = ap.resample_batch(wav[:1, :3000].contiguous(), [3000], 48000)
    assert n1 == [1379] and torch.equal(alone[0], out[0, :1379])


def test_a_target_other_than_the_processors_rate():
    ap = su.processor()
    (orig, target, N), = [c for c in ru.CASES if c[1] != 22050]
    assert (orig, target, N) == (22050, 16000, 2205)
    x, y = _case(orig, target, N)
    x2, y2 = _case(48000, 16000, 1000)
    wav, Ns = _ragged([x, x2])
    out, n_fix = ap.resample_batch(wav, Ns, [orig, 48000], target_sr=target)
    _check_rows(out, n_fix, [y, y2])


def test_caller_supplied_filter():
    ap = su.processor()
    filt = ru.small_filter()
    assert len(filt[0]) == 33 and filt[1] == 8
    x, y = _case(48000, 22050, 400, True)
    wav, N = _ragged([x])
    out, n_fix = ap.resample_batch(wav, N, 48000, res_type=filt)
    _check_rows(out, n_fix, [y])
    assert not _same(y, _case(48000, 22050, 400)[1])
    # the named filter is set again by the next call that asks for it
    x, y = _case(48000, 22050, 50)
    out, n_fix = ap.resample_batch(_ragged([x])[0], [50], 48000)
    _check_rows(out, n_fix, [y])


def test_a_chunk_smaller_than_the_workgroup():
    """22 050 -> 368 Hz: 60 inputs per output and wings of 4 096 taps each, so the staged window of 256
    outputs would not fit the 16 384 inputs a workgroup holds and the call runs 128 outputs per workgroup
    (two workgroups here)."""
    ap = su.processor()
    x, y = _case(22050, 368, 12000)
    assert len(y) == 201
    out, n_fix = ap.resample_batch(_ragged([x])[0], [12000], 22050, target_sr=368)
    _check_rows(out, n_fix, [y])


def test_padding_is_not_read_and_pitch_is_free():
    ap = su.processor()
    cases = [c for c in ru.CASES if c[1] == 22050]
    rows = [_case(*c) for c in cases]
    rates = [c[0] for c in cases]
    tight, N = _ragged([x for x, _ in rows])
    want, n_fix = ap.resample_batch(tight, N, rates)
    src, _ = _ragged([x for x, _ in rows], pitch=4003, fill=NAN)
    assert src.stride(0) % 2 == 1 and torch.isnan(src[0, 3000:]).all()
    dst = torch.full((len(N), 4501), NAN, dtype=torch.float64, device="cuda")
    st, msg, n_out = _raw(ap, src, N, rates, 22050, dst)
    assert st == 0, msg
    assert n_out == n_fix
    assert torch.isfinite(dst).all()
    assert torch.equal(dst[:, :want.shape[1]], want)
    res = [ru.lengths(n, r, 22050)[0] for n, r in zip(N, rates)]
    for b, n_res in enumerate(res):
        assert not dst[b, n_res:].any(), b
        assert dst[b, n_res - 1] != 0, b


def test_invalid_arguments_are_refused_before_any_launch():
    audio = load_pkg("audio")
    ap = su.processor()
    x = torch.from_numpy(np.tile(ru.signal(100, 48000).astype(np.float64), (2, 1))).cuda()
    dst = torch.full((2, 50), NAN, dtype=torch.float64, device="cuda")
    INVALID = 1  # TTS_ERR_INVALID

    def refused(pattern, src, N, rates, target, out, **kw):
        st, msg, _ = _raw(ap, src, N, rates, target, out, **kw)
        print(st, msg)
        assert st == INVALID
        assert re.search(pattern, msg), msg
        assert out is None or torch.isnan(out).all()  # nothing ran

    refused("no filter", x, [100, 100], [48000, 48000], 22050, dst)
    ap._set_resample_filter("kaiser_best")
    refused("null", None, [100, 100], [48000, 48000], 22050, dst)
    refused("null", x, [100, 100], [48000, 48000], 22050, None)
    refused("B must be positive", x, [100, 100], [48000, 48000], 22050, dst, B=0)
    refused("B must be positive", x, [100, 100], [48000, 48000], 22050, dst, B=-1)
    refused("target_sr", x, [100, 100], [48000, 48000], 0, dst)
    refused(r"sentence 1\b.*orig_sr", x, [100, 100], [48000, 0], 22050, dst)
    refused(r"sentence 1\b.*orig_sr", x, [100, 100], [48000, -8000], 22050, dst)
    refused(r"sentence 1\b.*src_pitch", x, [100, 0], [48000, 48000], 22050, dst)
    refused(r"sentence 1\b.*src_pitch", x, [100, 101], [48000, 48000], 22050, dst)
    refused(r"sentence 0\b.*src_pitch", x, [-5, 100], [48000, 48000], 22050, dst)
    refused(r"sentence 1\b.*too short", x, [100, 2], [48000, 48000], 22050, dst)  # n_res = int(0.91875) = 0
    refused(r"sentence 1\b.*dst_pitch", x, [100, 100], [48000, 44100], 22050, dst.new_full((2, 49), NAN))  # n_fix = 50
    refused(r"sentence 0\b.*dst_pitch", x, [100, 100], [16000, 48000], 22050, dst)  # n_fix = 138
    # ratio 0.008: step 4, wings of 32769 // 4 taps, more inputs than a workgroup stages
    long = torch.zeros(2, 1000, dtype=torch.float64, device="cuda")
    refused(r"sentence 1\b.*staging", long, [1000, 1000], [48000, 2756250], 22050, dst.new_full((2, 460), NAN))
    # a table with one entry per zero crossing: step = int(0.459 * 1) = 0 when downsampling
    lib, h = ap._handle()
    coarse = np.ascontiguousarray(np.linspace(1.0, 0.0, 9))
    assert lib.tts_gl_set_resample_filter(h, coarse.ctypes.data_as(ctypes.c_void_p), 9, 1) == 0
    refused(r"sentence 1\b.*step", x, [100, 100], [16000, 48000], 22050, dst.new_full((2, 200), NAN))
    assert lib.tts_gl_set_resample_filter(h, None, 9, 1) == INVALID
    assert lib.tts_gl_set_resample_filter(h, coarse.ctypes.data_as(ctypes.c_void_p), 0, 1) == INVALID
    assert lib.tts_gl_set_resample_filter(h, coarse.ctypes.data_as(ctypes.c_void_p), 9, 0) == INVALID
    with pytest.raises(ValueError):
        ap.resample_batch(x, [100, 2], 48000)
    with pytest.raises(NotImplementedError):
        ap.resample_batch(x, [100, 100], 48000, res_type="kaiser_fast")
    # the handle still serves a good call
    ap._resample_filter = None
    out, n_fix = ap.resample_batch(x[:, :50].contiguous(), [50, 50], 48000)
    _check_rows(out, n_fix, [_case(48000, 22050, 50)[1]] * 2)
    assert audio.resample_lengths(50, 48000, 22050) == (22, 23)


def _pcm(x):
    return np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)


def _voiced(N, sr, seed, lo, hi):
    """1e-4 noise with a 0.4 sine on [lo, hi) of N samples (fractions of N): something to trim."""
    rng = np.random.RandomState(seed)
    y = 1e-4 * rng.randn(N)
    t = np.arange(int(lo * N), int(hi * N))
    y[t] += 0.4 * np.sin(2 * np.pi * 300 * t / sr) + 0.1
    return y


def test_load_wav_resamples_a_stereo_file(tmp_path):
    N = 2400
    left = ru.signal(N, 48000).astype(np.float64)
    right = 0.7 * ru.signal(N, 48000)[::-1].astype(np.float64)
    pcm = np.stack([_pcm(left), _pcm(right)], axis=1)
    assert pcm.shape == (N, 2) and pcm.dtype == np.int16
    path = str(tmp_path / "stereo48.wav")
    scipy.io.wavfile.write(path, 48000, pcm)
    ap = su.processor(do_trim_silence=False)
    got = ap.load_wav(path, sr=22050)
    mono = ru.to_mono_f32(pcm / 32768.0)
    assert mono.dtype == np.float32 and not np.array_equal(mono, (pcm[:, 0] / 32768.0).astype(np.float32))
    want = ru.resample_ref(mono, 48000, 22050)
    assert got.dtype == np.float32 and len(got) == 1103
    assert _same(got, want)
    with pytest.raises(AssertionError):
        ap.load_wav(path, sr=16000)  # the reference's assert self.sample_rate == sr
    with pytest.raises(AssertionError):
        ap.load_wav(path)  # without sr nothing is resampled, as before


@pytest.mark.parametrize("trim", [False, True])
def test_load_wav_batch_resamples_mixed_files(tmp_path, trim, capsys):
    audio = load_pkg("audio")
    cfg = dict(su.tacotron2_config()["audio"])
    ap = audio.AudioProcessor(**{**cfg, "do_trim_silence": trim})
    paths = []
    for i, (sr, C) in enumerate([(48000, 2), (44100, 1), (22050, 1)]):
        N = int(0.45 * sr) + 17 * i
        chans = [_voiced(N, sr, 20 + i + c, 0.3 + 0.05 * i, 0.7 - 0.03 * c) for c in range(C)]
        paths.append(str(tmp_path / f"f{i}.wav"))
        scipy.io.wavfile.write(paths[-1], sr, _pcm(np.stack(chans, axis=1) if C > 1 else chans[0]))
    want = [ap.load_wav(p, sr=22050) for p in paths]
    assert all(w.dtype == np.float32 for w in want)
    wav, N = ap.load_wav_batch(paths, sr=22050)
    assert capsys.readouterr().out == ""
    print("samples", N)
    assert N == [len(w) for w in want] and wav.shape == (3, max(N)) and wav.dtype == torch.float64
    got = wav.cpu().numpy()
    for b, w in enumerate(want):
        assert np.array_equal(got[b, :N[b]], w), b
        assert not got[b, N[b]:].any(), b
    if trim:
        assert all(0 < n < 0.6 * 0.45 * 22050 for n in N)
    else:
        assert N[0] == 9923 and N[2] == int(0.45 * 22050) + 34
    # the analysis half takes the resident batch as it is
    mel, lin, F = ap.features_batch(wav, N)
    for b, w in enumerate(want):
        assert F[b] == 1 + len(w) // ap.hop_length
        assert np.array_equal(mel[b, :F[b]].T.double().cpu().numpy(), ap.melspectrogram(w)), b
        assert np.array_equal(lin[b, :F[b]].T.double().cpu().numpy(), ap.spectrogram(w)), b
    # without sr the batch call is what it was: a file at another rate is refused
    with pytest.raises(AssertionError):
        ap.load_wav_batch(paths)
