"""GPU parity of the resident batch decoder's general attention form (csrc/resident_batch.hip:
location features, windowing, transition agent): 2..8 sentences per request in persistent launches
of at most 4, each sentence with the reference's batch-1 semantics.

Against the reference's own runs (tests/golden/rbgen_*.npz at the kernel's length edges 2, 20, 33,
129, 256, and the full-length t2_loc_*_L100 fixtures): frame counts and stop decisions exact, the
per-step attention argmax by the argmax rule (rbgen_util.py), floats at the model-half tolerance.
Also: the multi-launch path on the same batches, bitwise determinism, the routing switches
(TTS_RB_GENERAL=0, a refused launch) and a constructor-default request through synthesis._decode.
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from rbgen_util import ALIGN_ATOL, assert_argmax, rbgen, rbgen_flags

pytestmark = pytest.mark.gpu
MEL_RTOL = 4e-6   # model half (test_gpu_resident_batch.py)
SAME_RTOL = 1e-5  # resident batch vs multi-launch / serial batch-1 calls: two fp32 reduction orders


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(fl, batch=True, max_batch=12, **env):
    """A model at flags fl whose native handles are created under TTS_RESIDENT_BATCH and env."""
    t2 = load_pkg("tacotron2")
    with _env(TTS_RESIDENT_BATCH="1" if batch else "0", **env):
        m = t2.Tacotron2(130, 0, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                         forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                         forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"],
                         max_batch=max_batch, max_len=256)
        m.decoder.max_decoder_steps = fl["max_decoder_steps"]
        m = m.cuda().eval()
        m.resident_limits(256)  # creates the native handles while the variables are set
    return m


def _run(m, encs):
    """encs: list of [L_b, 512] encoder outputs -> inference_batch on the padded batch."""
    lens = [e.shape[0] for e in encs]
    enc = torch.zeros(len(encs), max(lens), 512)
    for b, e in enumerate(encs):
        enc[b, :lens[b]] = torch.from_numpy(np.asarray(e, np.float32))
    return m.inference_batch(None, enc=enc.cuda(), lens=lens)


def _check(out, b, ref):
    """sentence b of a batch output vs a reference dict (mel, mel_post, align, stop)."""
    T = out["frames"][b]
    assert T == ref["mel"].shape[0], f"sentence {b}: {T} frames, reference {ref['mel'].shape[0]}"
    L = ref["align"].shape[1]
    al = out["align"][b, :T, :L].cpu().numpy()
    st = out["stop"][b, :T].cpu().numpy()
    mel, post = out["mel"][b, :T].cpu().numpy(), out["mel_post"][b, :T].cpu().numpy()
    print(f"sentence {b} L={L} T={T}: align {np.abs(al - ref['align']).max():.3g} stop {np.abs(st - ref['stop']).max():.3g} "
          f"mel {rel_rms(mel, ref['mel']):.3g} mel_post {rel_rms(post, ref['mel_post']):.3g}")
    assert_argmax(al, ref["align"], f"sentence {b}")
    assert np.abs(al - ref["align"]).max() < ALIGN_ATOL
    np.testing.assert_array_equal(st > 0.5, ref["stop"] > 0.5)
    assert np.abs(st - ref["stop"]).max() < ALIGN_ATOL
    assert rel_rms(mel, ref["mel"]) < MEL_RTOL
    assert rel_rms(post, ref["mel_post"]) < MEL_RTOL


def _check_same(a, b, lens, ref_aligns):
    """Two paths' outputs of one batch: equal frames, the argmax rule, floats at SAME_RTOL."""
    assert a["frames"] == b["frames"]
    for k, L in enumerate(lens):
        T = a["frames"][k]
        aa, ab = a["align"][k, :T, :L].cpu().numpy(), b["align"][k, :T, :L].cpu().numpy()
        assert_argmax(aa, ref_aligns[k], f"sentence {k} (first path)")
        assert_argmax(ab, ref_aligns[k], f"sentence {k} (second path)")
        assert np.abs(aa - ab).max() < SAME_RTOL
        sa, sb = a["stop"][k, :T].cpu().numpy(), b["stop"][k, :T].cpu().numpy()
        np.testing.assert_array_equal(sa > 0.5, sb > 0.5)
        for key in ("mel", "mel_post"):
            assert rel_rms(a[key][k, :T].cpu().numpy(), b[key][k, :T].cpu().numpy()) < SAME_RTOL, (k, key)


def _fix(name):
    z = golden(name)
    return dict(enc=z["enc"], mel=z["mel"], mel_post=z["mel_post"], align=z["align"], stop=z["stop"])


@pytest.mark.parametrize("config", ["loc_softmax", "loc_fwd_ta", "loc_fwd_ta_mask", "win_fwdmask", "win_softmax"])
def test_general_batch_vs_reference(config):
    """Every configuration in one launch of 4 at the lengths 129 (past the LDS context copy), 2, 33, 20."""
    m = _model(rbgen_flags(config))
    refs = [rbgen(config, L) for L in (129, 2, 33, 20)]
    out = _run(m, [r["enc"] for r in refs])
    assert m.last_timing["resident_kind"] == 2, "the resident batch decoder did not serve this batch"
    for b, r in enumerate(refs):
        _check(out, b, r)


@pytest.mark.parametrize("lens", [
    [256, 2],                             # the NB = 2 kernel with the whole context in LDS, 8 positions per wave
    [20, 129, 33],                        # NB = 4 beside a padding sentence
    [20, 2, 33, 20, 129],                 # 4 + 1: the last launch holds one sentence, unlike the four before
    [256, 2, 33, 20, 129, 256, 20, 33],   # 4 + 4 with a 256 in each group
], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("config", ["loc_softmax", "loc_fwd_ta"])
def test_general_batch_group_shapes(config, lens):
    m = _model(rbgen_flags(config))
    refs = [rbgen(config, L) for L in lens]
    out = _run(m, [r["enc"] for r in refs])
    assert m.last_timing["resident_kind"] == 2
    for b, r in enumerate(refs):
        _check(out, b, r)


@pytest.mark.parametrize("config", ["loc_fwd_ta_mask", "win_softmax"])
def test_general_batch_vs_multilaunch(config):
    """The same handle created under TTS_RESIDENT_BATCH=0 (the multi-launch location / windowing
    step at B <= 8) on the same batch."""
    fl = rbgen_flags(config)
    res, ml = _model(fl, True), _model(fl, False)
    lens = (129, 2, 33, 20)
    refs = [rbgen(config, L) for L in lens]
    a = _run(res, [r["enc"] for r in refs])
    assert res.last_timing["resident_kind"] == 2
    b = _run(ml, [r["enc"] for r in refs])
    assert ml.last_timing["resident_kind"] == 0
    _check_same(a, b, lens, [r["align"] for r in refs])


@pytest.mark.parametrize("case", ["t2_loc_softmax_L100", "t2_loc_fwd_ta_L100"])
def test_general_batch_full_length(case):
    """The full-length runs (300 steps under softmax; 222 frames with the transition agent), two
    copies per launch."""
    z = golden(case)
    m = _model(golden_flags(z))
    out = _run(m, [z["enc"], z["enc"]])
    assert m.last_timing["resident_kind"] == 2
    for b in range(2):
        _check(out, b, _fix(case))


def test_general_batch_deterministic():
    m = _model(rbgen_flags("loc_fwd_ta"))
    encs = [rbgen("loc_fwd_ta", L)["enc"] for L in (33, 129, 20)]
    a = _run(m, encs)
    b = _run(m, encs)
    assert m.last_timing["resident_kind"] == 2
    assert a["frames"] == b["frames"]
    for k in ("mel", "mel_post", "align", "stop"):
        assert torch.equal(a[k], b[k]), k


def test_general_batch_switch_keeps_the_other_routing():
    """TTS_RB_GENERAL=0 at create: a location batch runs multi-launch; synthesize.py's configuration
    on a handle made the same way is still served by the resident batch decoder."""
    m = _model(rbgen_flags("loc_softmax"), TTS_RB_GENERAL=0)
    _run(m, [rbgen("loc_softmax", L)["enc"] for L in (33, 20)])
    assert m.last_timing["resident_kind"] == 0
    cases = ["t2_fwdmask_L12", "t2_fwdmask_L40"]
    m = _model(golden_flags(golden(cases[0])), TTS_RB_GENERAL=0)
    _run(m, [golden(c)["enc"] for c in cases])
    assert m.last_timing["resident_kind"] == 2


def test_general_batch_not_launched_reruns_multilaunch():
    """Under TTS_CU_CAP the launch is refused, nothing runs on the device and the batch starts again
    on the multi-launch path, bitwise that path's output."""
    fl = rbgen_flags("loc_softmax")
    encs = [rbgen("loc_softmax", L)["enc"] for L in (33, 2, 20)]
    want = _run(_model(fl, False, max_batch=4), encs)
    fb = _model(fl, True, max_batch=4)
    assert fb.resident_limits(256)[0] == 4
    with _env(TTS_CU_CAP=8):
        got = _run(fb, encs)
        assert fb.last_timing["resident_kind"] == 0
    assert got["frames"] == want["frames"]
    for k in ("mel", "mel_post", "align", "stop"):
        assert torch.equal(got[k], want[k]), k


def test_constructor_default_request_is_batch_resident():
    """synthesis._decode on a constructor-default model (location-sensitive attention + softmax,
    models/tacotron2.py:17,23): 3 sentences go to the resident batch decoder, and agree with the
    serial batch-1 calls the same request takes under TTS_RB_GENERAL=0."""
    t2, syn = load_pkg("tacotron2"), load_pkg("synthesis")
    w = weights_mod()
    ids = [w.synthetic_ids(L, seed) for L, seed in ((20, 922), (33, 935), (2, 902))]
    outs = []
    for env, dispatch in ((dict(), "batch-resident"), (dict(TTS_RB_GENERAL=0), "serial-resident")):
        with _env(**env):
            m = t2.Tacotron2(130, 0, max_batch=8)
            m.decoder.max_decoder_steps = 60
            m = m.cuda().eval()
            out = syn._decode(m, ids)
        assert out["dispatch"] == dispatch
        outs.append(out)
    assert m.flags["location_attn"] and m.flags["attn_norm"] == "softmax" and not m.flags["forward_attn"]
    lens = [len(x) for x in ids]
    _check_same(outs[0], outs[1], lens, [rbgen("loc_softmax", L)["align"] for L in lens])
