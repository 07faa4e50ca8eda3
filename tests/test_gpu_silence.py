"""GPU: silence trimming and endpoint detection on the device (tts_gl_trim_silence, tts_gl_find_endpoint,
tts_gl_take_segments; AudioProcessor.trim_silence_batch / find_endpoint_batch / take_segments /
load_wav_batch; synthesize_batch(trim_silence=True)) against the host AudioProcessor.trim_silence and
find_endpoint.  Every integer is compared exactly; test_silence_cpu.py shows why the inputs allow that."""
import numpy as np
import pytest
import scipy.io.wavfile
import torch

import silence_util as su
from conftest import golden, load_pkg, weights_mod

pytestmark = pytest.mark.gpu


def _loud(b, count):  # padding behind a sentence: a read past N[b] changes the loudest frame
    return 100.0 * np.where(np.arange(count) % 2 == 0, 1.0, -1.0)


def _alternating(b, count):  # -100, +100, ...: a read past N[b] shows under the signed maximum
    return 100.0 * np.where(np.arange(count) % 2 == 0, -1.0, 1.0)


def _example_pcm():
    return golden("audio_example1")["pcm"].astype(np.float64) / 32768.0


def test_trim_parity_ragged_batch():
    ap = su.processor(su.TRIM_SR)
    margin = 200
    wavs = su.trim_wavs(margin)
    host, N = su.ragged(wavs, _loud)
    assert len(N) == 10 and len(set(N)) > 5 and N == [len(y) + 400 for y in su.trim_signals()]
    dev = torch.from_numpy(host).cuda()
    want = [su.host_trim_bounds(ap, w) for w in wavs]
    start, end = ap.trim_silence_batch(dev, N)
    print("device", list(zip(start, end)), "host", want)
    assert list(zip(start, end)) == want
    assert ap.trim_silence_batch(dev, N) == (start, end)
    lens = [e - s for s, e in zip(start, end)]
    seg = ap.take_segments(dev, [margin + s for s in start], lens)
    assert seg.shape == (10, max(lens)) and seg.dtype == torch.float64
    seg = seg.cpu().numpy()
    for b, w in enumerate(wavs):
        assert np.array_equal(seg[b, :lens[b]], ap.trim_silence(w)), b
        assert not seg[b, lens[b]:].any(), b


def test_trim_real_audio_alone_and_in_a_batch():
    ap = su.processor()
    assert ap.sample_rate == 22050
    y = _example_pcm()
    assert len(y) == 41885
    want = su.host_trim_bounds(ap, y)
    start, end = ap.trim_silence_batch(torch.from_numpy(y).cuda()[None], [len(y)])
    print("device", (start, end), "host", want)
    assert (start[0], end[0]) == want
    rng = np.random.RandomState(7)
    others = [su.with_margins(s, 2205, rng) for s in su.trim_signals()[5:7]]
    rows = [others[0], others[1], y]
    host, N = su.ragged(rows, _loud)
    start, end = ap.trim_silence_batch(torch.from_numpy(host).cuda(), N)
    assert list(zip(start, end)) == [su.host_trim_bounds(ap, r) for r in rows]
    assert (start[2], end[2]) == want


def test_trim_refuses_short_sentences_before_any_launch():
    ap = su.processor(su.TRIM_SR)
    sigs = su.trim_signals()
    rng = np.random.RandomState(7)
    rows = [su.with_margins(sigs[1], 200, rng), su.with_margins(sigs[0][:512], 200, rng)]
    host, N = su.ragged(rows, _loud)
    assert N[1] - 400 == 512
    dev = torch.from_numpy(host).cuda()
    with pytest.raises(RuntimeError, match=r"sentence 1\b"):
        ap.trim_silence_batch(dev, N)
    with pytest.raises(RuntimeError, match=r"sentence 0\b.*margins"):
        ap.trim_silence_batch(dev, [399, N[1]])
    with pytest.raises(RuntimeError, match="pitch"):
        ap.trim_silence_batch(dev, [N[0], host.shape[1] + 1])
    # the handle still serves a good call
    assert ap.trim_silence_batch(dev[:1], N[:1]) == ([0], [1024])


@pytest.mark.parametrize("sec,window", [(0.8, 800), (0.801, 801)])
def test_endpoint_parity_ragged_batch(sec, window):
    ap = su.processor(su.END_SR)
    cases = su.endpoint_cases(ap, sec)
    want = [ap.find_endpoint(y, min_silence_sec=sec) for y in cases]
    host, N = su.ragged(cases, _alternating)
    dev = torch.from_numpy(host).cuda()
    got = ap.find_endpoint_batch(dev, N, min_silence_sec=sec)
    print("device", got, "host", want)
    assert got == want
    assert ap.find_endpoint_batch(dev, N, min_silence_sec=sec) == got
    # a batch in which no sentence has a candidate
    short = [b for b, n in enumerate(N) if n <= window + 200]
    assert len(short) == 3
    assert ap.find_endpoint_batch(dev[short].contiguous(), [N[b] for b in short], min_silence_sec=sec) == \
        [N[b] for b in short]


def test_take_segments_refuses_bad_ranges():
    ap = su.processor(su.TRIM_SR)
    dev = torch.zeros(2, 100, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=r"sentence 1\b.*src_pitch"):
        ap.take_segments(dev, [0, 51], [100, 50])
    with pytest.raises(RuntimeError, match="negative"):
        ap.take_segments(dev, [-1, 0], [10, 10])


def test_load_wav_batch(tmp_path, capsys):
    audio_cfg = dict(su.tacotron2_config()["audio"])
    pcm = golden("audio_example1")["pcm"]
    rng = np.random.RandomState(7)
    synth = su.with_margins(0.3 * su.trim_signals()[6], 2205, rng)
    synth = np.clip(synth * 0.05, -1, 1)
    short = 0.1 * np.sin(0.05 * np.arange(2 * 2205 + 512))
    paths = []
    for name, x in (("example", pcm), ("synth", (synth * 32767).astype(np.int16)),
                    ("short", (short * 32767).astype(np.int16))):
        paths.append(str(tmp_path / (name + ".wav")))
        scipy.io.wavfile.write(paths[-1], 22050, x)
    audio = load_pkg("audio")
    ap_trim = audio.AudioProcessor(**{**audio_cfg, "do_trim_silence": True})
    ap_raw = audio.AudioProcessor(**{**audio_cfg, "do_trim_silence": False})
    raw = [ap_raw.load_wav(p) for p in paths]
    assert len(raw[2]) == 2 * 2205 + 512
    want = [ap_trim.load_wav(paths[0]), ap_trim.load_wav(paths[1]), raw[2]]  # the short file stays whole
    assert len(want[0]) < len(raw[0]) and len(want[1]) < len(raw[1])
    capsys.readouterr()
    wav, N = ap_trim.load_wav_batch(paths)
    assert capsys.readouterr().out == f" [!] File cannot be trimmed for silence - {paths[2]}\n"
    assert N == [len(w) for w in want] and wav.shape == (3, max(N)) and wav.dtype == torch.float64
    got = wav.cpu().numpy()
    for b, w in enumerate(want):
        assert np.array_equal(got[b, :N[b]], w), b
        assert not got[b, N[b]:].any(), b
    # untrimmed
    wav_raw, N_raw = ap_raw.load_wav_batch(paths)
    assert capsys.readouterr().out == ""
    assert N_raw == [len(w) for w in raw]
    got_raw = wav_raw.cpu().numpy()
    for b, w in enumerate(raw):
        assert np.array_equal(got_raw[b, :N_raw[b]], w), b
    # the analysis entry points take the result as it is
    host, _ = su.ragged(want, lambda b, count: np.zeros(count))
    mel, lin, F = ap_trim.features_batch(wav, N)
    mel_h, lin_h, F_h = ap_trim.features_batch(torch.from_numpy(host).cuda(), [len(w) for w in want])
    assert F == F_h and torch.equal(mel, mel_h) and torch.equal(lin, lin_h)


def test_synthesize_batch_trim_silence(audio_cfg):
    gu = load_pkg("generic_utils")
    cfg = gu.default_config("config_tacotron2.json")
    cfg.forward_attn_mask = True  # synthesize.py:86
    m = gu.setup_model(130, cfg, max_batch=4, max_len=256).cuda().eval()
    w = weights_mod()
    ids = [w.synthetic_ids(L, 100 + b) for b, L in enumerate((40, 64, 52))]
    ap = load_pkg("audio").AudioProcessor(**audio_cfg)
    syn = load_pkg("synthesis").synthesize_batch
    base, info0 = syn(m, ap, ids, seed=3, iters=2, keep_outputs=True)
    same, info1 = syn(m, ap, ids, seed=3, iters=2, keep_outputs=True, trim_silence=False)
    assert info1["samples"] == info0["samples"] == [ap.hop_length * (T - 1) for T in info0["frames"]]
    assert all(np.array_equal(a, b) for a, b in zip(base, same))
    # (the windows are 17 640 samples, the hop 4 410: every sentence has candidates)
    assert min(info0["samples"]) > 17640 + 4410
    wavs, info = syn(m, ap, ids, seed=3, iters=2, keep_outputs=True, trim_silence=True)
    full = info["wav_dev"].cpu().numpy()
    assert np.array_equal(full, info0["wav_dev"].cpu().numpy())
    want = [ap.find_endpoint(full[b, :n]) for b, n in enumerate(info0["samples"])]
    print("device", info["samples"], "host", want)
    assert info["samples"] == want
    for b, n in enumerate(want):
        assert np.array_equal(wavs[b], full[b, :n]), b
    none, info_dev = syn(m, ap, ids, seed=3, iters=2, to_host=False, trim_silence=True)
    assert none is None and info_dev["samples"] == want
    pcm = ap.pcm16_join(info_dev["wav_dev"], info_dev["samples"], gap=10000)
    assert pcm.dtype == np.int16 and len(pcm) == sum(want) + 3 * 10000
