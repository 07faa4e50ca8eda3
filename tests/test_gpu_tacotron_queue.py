"""GPU parity of the Tacotron / TacotronGST decoder memory queue (memory_size > r) and of the
teacher-forced decoder (Decoder.forward, Tacotron.forward, TacotronGST.forward) against the
reference's own runs (tests/golden/tmq_*.npz, ttf_*.npz, made by
tests/golden/make_golden_tacotron_queue.py), the torch oracle, and themselves across batch shapes
and serving paths.

Tolerances are those of tests/test_gpu_tacotron.py: step counts, per-step attention argmax and the
stop decisions exact; alignments and stop values max-abs 4e-6; mel / linear relative RMS 4e-6."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod

pytestmark = pytest.mark.gpu

RTOL = 4e-6
ATOL = 4e-6

# case -> served by the resident decoder (queue of at most 512 values, config_tacotron_gst.json's attention)
QUEUE_CASES = {
    "tmq_gst_r2_m5_L10": True,
    "tmq_gst_r1_m5_L4": True,
    "tmq_gst_r3_m5_L24_spk": True,
    "tmq_gst_r5_m6_L10": True,
    "tmq_gst_r2_m5_L10_prenetbn": True,    # prenet_type "bn": the BatchNorm fold over the 400-wide queue
    "tmq_taco_r2_m8_L10_loc": False,       # 640 wide, location attention
    "tmq_taco_r4_m5_L12_softmax": False,   # softmax attention
}
TEACHER_CASES = ["ttf_gst_r5_m5_L12", "ttf_gst_r2_m5_L12", "ttf_taco_r2_m8_L10_loc_ta"]
RAGGED_LENS = [10, 2, 4, 7, 10]  # two XCD groups of the resident decoder, the second with one sentence


def _model(fl, **kw):
    t = load_pkg("tacotron")
    cls = t.TacotronGST if fl["model"] == "TacotronGST" else t.Tacotron
    m = cls(130, fl["num_speakers"], r=fl["r"], memory_size=fl["memory_size"], attn_win=fl["attn_win"],
            attn_norm=fl["attn_norm"], forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
            forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"],
            prenet_type=fl.get("prenet_type", "original"), **kw)
    m.decoder.max_decoder_steps = fl["max_decoder_steps"]
    return m.cuda().eval()


def _check_decoder(mel, align, stop, ref_mel, ref_align, ref_stop, L):
    assert align.shape[0] == ref_align.shape[0], "step count differs"
    assert mel.shape == ref_mel.shape
    np.testing.assert_array_equal(align[:, :L].argmax(1), ref_align[:, :L].argmax(1))
    assert np.abs(align[:, :L] - ref_align[:, :L]).max() < ATOL
    np.testing.assert_array_equal(stop > 0.6, ref_stop > 0.6)
    assert np.abs(stop - ref_stop).max() < ATOL
    assert rel_rms(mel, ref_mel) < RTOL


def _np(out, b=0):
    """Sentence b of an inference_batch result as numpy (mel, align, stop), trimmed to its steps."""
    T, S = out["frames"][b], out["steps"][b]
    return out["mel"][b, :T].cpu().numpy(), out["align"][b, :S].cpu().numpy(), out["stop"][b, :S].cpu().numpy()


# ------------------------------------------------------------------ 1. reference fixtures, both paths
@pytest.mark.parametrize("resident", ["default", "off"])
@pytest.mark.parametrize("case", sorted(QUEUE_CASES))
def test_queue_inference_vs_reference(case, resident, monkeypatch):
    if resident == "off":
        monkeypatch.setenv("TTS_RESIDENT", "0")  # read when the handle is created
    z = golden(case)
    fl = golden_flags(z)
    m = _model(fl)
    sid = int(z["speaker_id"])
    kw = dict(speaker_ids=None if sid < 0 else torch.tensor([sid]))
    if fl["model"] == "TacotronGST":
        kw["style_mel"] = torch.from_numpy(z["style_mel"])[None] if "style_mel" in z else None
    mel, lin, align, stop = m.inference(torch.from_numpy(z["ids"])[None], **kw)
    assert m.last_timing["resident"] is (QUEUE_CASES[case] and resident == "default")
    assert stop.shape == (1, z["align"].shape[0]) and lin.shape[1:] == (z["mel"].shape[0], 1025)
    _check_decoder(mel[0].cpu().numpy(), align[0].cpu().numpy(), stop[0].cpu().numpy(), z["mel"], z["align"],
                   z["stop"], len(z["ids"]))
    if "linear" in z:
        assert rel_rms(lin[0].cpu().numpy(), z["linear"]) < RTOL


# ------------------------------------------------------------------ 2-4. r = 2, memory_size = 5 across paths / batches
@pytest.fixture(scope="module")
def r2m5():
    """One r=2 / memory_size=5 GST model per serving path, the ragged batch, and each path's results:
    the batch and every sentence alone."""
    w = weights_mod()
    fl = golden_flags(golden("tmq_gst_r2_m5_L10"))
    ids = [w.synthetic_ids(L, 300 + b) for b, L in enumerate(RAGGED_LENS)]
    res = {}
    mp = pytest.MonkeyPatch()
    try:
        for path in ("default", "off"):
            if path == "off":
                mp.setenv("TTS_RESIDENT", "0")
            m = _model(fl)
            batch = m.inference_batch(ids)
            batch_res = m.last_timing["resident"]
            single = []
            for x in ids:
                single.append(m.inference_batch([x]))
                assert m.last_timing["resident"] is batch_res
            res[path] = dict(model=m, batch=batch, single=single, resident=batch_res)
    finally:
        mp.undo()
    return dict(fl=fl, ids=ids, **res)


def test_queue_paths_serve_as_documented(r2m5):
    assert r2m5["default"]["resident"] is QUEUE_CASES["tmq_gst_r2_m5_L10"]
    assert r2m5["off"]["resident"] is False


def test_queue_resident_vs_multilaunch(r2m5):
    a, b = r2m5["default"], r2m5["off"]
    assert a["batch"]["steps"] == b["batch"]["steps"]
    assert min(a["batch"]["steps"]) >= 1 and max(a["batch"]["steps"]) >= 2
    for i, L in enumerate(RAGGED_LENS):
        _check_decoder(*_np(a["batch"], i), *_np(b["batch"], i), L)
        _check_decoder(*_np(a["single"][i]), *_np(b["single"][i]), L)
        T = a["batch"]["frames"][i]
        assert rel_rms(a["batch"]["linear"][i, :T].cpu().numpy(), b["batch"]["linear"][i, :T].cpu().numpy()) < RTOL


@pytest.mark.parametrize("path", ["default", "off"])
def test_queue_ragged_batch_matches_batch1(r2m5, path):
    r = r2m5[path]
    out = r["batch"]
    assert out["steps"] == [s["steps"][0] for s in r["single"]]
    for i, L in enumerate(RAGGED_LENS):
        _check_decoder(*_np(out, i), *_np(r["single"][i]), L)
        T, S = out["frames"][i], out["steps"][i]
        assert torch.all(out["mel"][i, T:] == 0), "mel rows past the sentence's frames must be zero"
        assert torch.all(out["linear"][i, T:] == 0)


def test_queue_ragged_batch_vs_torch_oracle(r2m5):
    from oracle.tacotron_torch import TacotronTorchCPU
    fl = r2m5["fl"]
    o = TacotronTorchCPU(weights_mod().tacotron_gst_weights(0, r=fl["r"], memory_size=fl["memory_size"]), **fl)
    for i in (2, 3):
        ref = o.inference(r2m5["ids"][i])
        for path in ("default", "off"):
            _check_decoder(*_np(r2m5[path]["batch"], i), ref["mel"], ref["align"], ref["stop"], RAGGED_LENS[i])


@pytest.mark.parametrize("path", ["default", "off"])
def test_queue_is_reinitialised_between_calls(r2m5, path):
    """The queue restarts from memory_init on every call: a repeated call is bit-identical, and a
    shorter batch after a longer one gets what it got on its own."""
    r = r2m5[path]
    m, ids = r["model"], r2m5["ids"]
    again = m.inference_batch(ids)
    assert again["steps"] == r["batch"]["steps"]
    for k in ("mel", "linear"):
        assert torch.equal(again[k], r["batch"][k]), k
    for i in range(len(ids)):  # (stop / align rows past a sentence's steps are not part of the result)
        for x, y in zip(_np(again, i), _np(r["batch"], i)):
            np.testing.assert_array_equal(x, y)
    short = m.inference_batch([ids[2]])
    assert short["steps"] == r["single"][2]["steps"]
    for k in ("mel", "align", "stop"):
        assert torch.equal(short[k], r["single"][2][k]), k


def test_queue_resident_timeout_rerun_and_phases(r2m5, monkeypatch):
    """The resident decoder's bounded waits (tests/test_gpu_tacotron.py's injection, TTS_DEC_WAIT_TICKS=1):
    a queue model's batch re-runs on the multi-launch path from memory_init, bitwise that path's
    output; and the phase-timer re-run of a resident queue batch works."""
    assert r2m5["default"]["resident"] is True
    ids = r2m5["ids"]
    monkeypatch.setenv("TTS_DEC_WAIT_TICKS", "1")
    mt = _model(r2m5["fl"])
    got = mt.inference_batch(ids)
    assert mt.last_timing["resident"] is False, "no timeout was injected"
    want = r2m5["off"]["batch"]
    assert got["steps"] == want["steps"]
    for i in range(len(ids)):  # (stop / align rows past a sentence's steps are not part of the result)
        for x, y in zip(_np(got, i), _np(want, i)):
            np.testing.assert_array_equal(x, y)
    m = r2m5["default"]["model"]
    m.inference_batch(ids)
    ph = m.profile_resident_phases()
    assert set(ph) == {"cu0", "cu1"} and all(v >= 0 for v in ph["cu0"].values())
    assert 1.0 < sum(ph["cu0"].values()) < 200.0  # microseconds per step


# ------------------------------------------------------------------ 5. teacher forcing vs the reference
@pytest.mark.parametrize("case", TEACHER_CASES)
def test_teacher_forcing_vs_reference(case):
    z = golden(case)
    fl = golden_flags(z)
    m = _model(fl)
    L, r = len(z["ids"]), fl["r"]
    teacher = torch.from_numpy(z["teacher"])[None]
    mel, align, stop = m.decoder_forward(torch.from_numpy(z["enc"])[None], teacher)
    assert m.last_timing["resident"] is False
    steps = z["teacher"].shape[0] // r
    assert mel.shape == (1, steps, 80 * r) and align.shape == (1, steps, L) and stop.shape == (1, steps)
    _check_decoder(mel[0].reshape(-1, 80).cpu().numpy(), align[0].cpu().numpy(), stop[0].cpu().numpy(),
                   z["mel"], z["align"], z["stop"], L)
    mel2, lin, align2, stop2 = m.forward(torch.from_numpy(z["ids"])[None], [L], teacher)
    assert m.last_timing["resident"] is False
    assert mel2.shape == (1, steps * r, 80) and lin.shape == (1, steps * r, 1025)
    _check_decoder(mel2[0].cpu().numpy(), align2[0].cpu().numpy(), stop2[0].cpu().numpy(), z["mel"], z["align"],
                   z["stop"], L)
    assert rel_rms(lin[0].cpu().numpy(), z["linear"]) < RTOL


# ------------------------------------------------------------------ 6. free running == teacher forced on its own output
def test_teacher_forcing_reproduces_free_run(r2m5):
    m = r2m5["off"]["model"]
    x = golden("tmq_gst_r2_m5_L10")["ids"]
    L = len(x)
    enc = m.encode(torch.from_numpy(x)[None].cuda(), [L])
    free = m.inference_batch(None, enc=enc, lens=[L], postnet=False)
    fmel, falign, fstop = _np(free)
    assert free["steps"][0] == 30  # far past the three steps memory_init stays in the queue
    mel, align, logits = m.decoder_forward(enc, free["mel"][:, :free["frames"][0]])
    _check_decoder(mel[0].reshape(-1, 80).cpu().numpy(), align[0].cpu().numpy(),
                   torch.sigmoid(logits[0]).cpu().numpy(), fmel, falign, fstop, L)


# ------------------------------------------------------------------ 7. teacher forcing, ragged batch
def test_teacher_forcing_ragged_batch_matches_batch1(r2m5):
    m = r2m5["off"]["model"]
    lens = [10, 4, 7]
    ids = [r2m5["ids"][i] for i in (0, 2, 3)]
    x = torch.zeros(3, 10, dtype=torch.long)
    for b, s in enumerate(ids):
        x[b, :lens[b]] = torch.from_numpy(s)
    enc = m.encode(x.cuda(), lens)
    teacher = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(0, 1, (3, 16, 80)).astype(np.float32))
    mask = torch.arange(10)[None, :] < torch.tensor(lens)[:, None]
    mel, align, stop = m.decoder_forward(enc, teacher, mask)
    assert mel.shape == (3, 8, 160) and align.shape == (3, 8, 10) and stop.shape == (3, 8)
    for b, L in enumerate(lens):
        mel1, align1, stop1 = m.decoder_forward(enc[b:b + 1, :L], teacher[b:b + 1])
        _check_decoder(mel[b].cpu().numpy(), align[b].cpu().numpy(), stop[b].cpu().numpy(), mel1[0].cpu().numpy(),
                       align1[0].cpu().numpy(), stop1[0].cpu().numpy(), L)
    with pytest.raises(ValueError):
        m.decoder_forward(enc, teacher[:, :15])  # T % r != 0


def test_teacher_forcing_ignores_rows_it_does_not_consume(r2m5):
    """The last step's [prenet L1 | stopnet] launch still reads a queue window ending in history row
    steps-1, which no step consumes: whatever an earlier call left there (here NaN teacher frames)
    must not reach the stop logit."""
    m = r2m5["off"]["model"]
    x = r2m5["ids"][3]
    enc = m.encode(torch.from_numpy(x)[None].cuda(), [len(x)])
    clean = torch.from_numpy(np.random.Generator(np.random.PCG64(6)).uniform(0, 1, (1, 16, 80)).astype(np.float32))
    want = m.decoder_forward(enc, clean[:, :10])       # 5 steps: teacher rows 0..3 are read
    poison = clean.clone()
    poison[:, 8:10] = float("nan")                     # row 4 of an 8-step call lands in the history
    m.decoder_forward(enc, poison)
    got = m.decoder_forward(enc, clean[:, :10])
    for g, w in zip(got, want):
        assert torch.isfinite(g).all()
        assert torch.equal(g, w)
    one = m.decoder_forward(enc, clean[:, :2])         # one step: the whole window is memory_init + row 0
    assert all(torch.isfinite(v).all() for v in one)
    assert torch.equal(one[0][:, 0], want[0][:, 0]) and torch.equal(one[2][:, 0], want[2][:, 0])


def test_forward_keeps_one_handle_for_a_long_teacher(r2m5):
    """A teacher longer than max_decoder_steps + 1 steps needs a larger handle once, not per stage."""
    m = _model(r2m5["fl"])
    m.decoder.max_decoder_steps = 4
    x = r2m5["ids"][2]
    teacher = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).uniform(0, 1, (1, 24, 80)).astype(np.float32))
    out = m.forward(torch.from_numpy(x)[None], [len(x)], teacher)          # 12 steps > 5
    h = m._native[0].value
    assert m._native[1][0] == 11
    again = m.forward(torch.from_numpy(x)[None], [len(x)], teacher)
    assert m._native[0].value == h, "the handle was re-created"
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    m.inference(torch.from_numpy(x)[None])                                 # the free-running decoder wants its own cap
    assert m._native[1][0] == 4


# ------------------------------------------------------------------ 8. argument checks of the C-ABI
def test_abi_argument_checks(r2m5):
    n = load_pkg("_native")
    lib = n.lib()
    m = r2m5["off"]["model"]
    w = {k: v.float().contiguous() for k, v in m._params.items() if v.is_floating_point()}
    arr, keep = n.tensor_views(w)
    cfg = n.TacotronConfig(r=5, memory_size=3, attn_norm=1, forward_attn=1, trans_agent=0, forward_attn_mask=0,
                           location_attn=0, windowing=0, gst=1, num_speakers=0, max_batch=1, max_len=16, max_steps=8)
    h = ctypes.c_void_p()
    assert lib.tts_tacotron_create(ctypes.byref(cfg), arr, len(w), n.stream_handle(), ctypes.byref(h)) == 1
    assert b"memory_size" in lib.tts_last_error()
    # teacher forcing on the live handle (history capacity max_decoder_steps + 1 = 41 steps)
    _, hd = m._handle(10, 1)
    cap = int(m.decoder.max_decoder_steps) + 1
    enc = torch.zeros(1, 10, 256, device="cuda")
    steps = cap + 1
    mem = torch.zeros(1, steps * 160, device="cuda")
    mel = torch.zeros(1, steps, 160, device="cuda")
    stop = torch.zeros(1, steps, device="cuda")

    def call(steps, ldb):
        return lib.tts_tacotron_decode_teacher(hd, ctypes.c_void_p(enc.data_ptr()), n.i32_array([10]), 1, 10,
                                               ctypes.c_void_p(mem.data_ptr()), ldb, steps,
                                               ctypes.c_void_p(mel.data_ptr()), ctypes.c_void_p(stop.data_ptr()),
                                               None, n.stream_handle())
    assert call(cap + 1, steps * 160) == 1   # beyond the history capacity
    assert call(4, 3 * 160 - 1) == 1         # rows shorter than the teacher frames the steps read
    assert call(4, 3 * 160) == 0
    torch.cuda.synchronize()
