"""GPU: the resident batch-1 decoder's energy-partials hand-off (csrc/resident_decoder.hip, synthesis
configuration).  Every CU of an XCD forms one lane's partial of the <= 15 candidate energies from the
four query rows it holds, publishes 16 partials, gathers the XCD's 16 x 32 and finishes the attention
step itself: no query gather on one attention CU, no context hand-off.  The floating-point
expressions and their order are those of the form before it, so the outputs must not move by a bit.

1. Bitwise against the fixture tests/golden/resident_energy_partials.npz: resident mel, align, stop
   and frames of the t2_fwdmask configuration for synthetic_ids(L, 300 + L), L in {16, 100, 256},
   written by the build of commit e01191b (the last one with an attention CU per XCD), not by the
   code under test.  L = 16 is the smallest length at which all 15 candidate slots are distinct
   positions, L = 100 the benchmark's, L = 256 = RES_LMAX reaches the last column of Pt and 534 steps.
2. One handle across step parities: max_decoder_steps 5, 6, a full L = 12 run, 5 again; each equals
   the same run on a fresh handle bit for bit (partial granules left by another launch or parity).
3. Resident against multi-launch at L = 33: exact frames, equal alignment argmax, mel relative RMS
   below SAME_RTOL = 1e-5 (the project's bound for the same fp32 step in two reduction orders,
   test_gpu_resident.py).
4. The full evaluation at a step t > 0 (every candidate's unnormalised weight below 1e-8) has no case:
   a CPU search with Tacotron2Oracle (fp32) over synthetic_ids(L, s), L in 2..16, s in 300..400,
   found none.  The smallest row maximum over all their steps t > 0 is 0.163 (L = 16, s = 316,
   t = 13).  These weights cannot reach it at any sentence: |e| <= ||v||_1 + |b_v| = 13.9, so
   sigmoid(e) >= 9e-7, and the position holding the largest previous weight (>= 1/6 over the six
   the mask keeps) has mix >= 1/12: the row maximum stays above 7e-8.  The branch is exercised at
   step 0 only (every case here starts with it)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod

pytestmark = pytest.mark.gpu

LENGTHS = [16, 100, 256]
KEYS = ("mel", "align", "stop")
SAME_RTOL = 1e-5


def _model(fl, resident, max_steps=None):
    """A model whose native handles are created under TTS_RESIDENT = resident."""
    t2 = load_pkg("tacotron2")
    old = os.environ.get("TTS_RESIDENT")
    os.environ["TTS_RESIDENT"] = "1" if resident else "0"
    try:
        m = t2.Tacotron2(130, 0, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                         forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                         forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"])
        m.decoder.max_decoder_steps = fl["max_decoder_steps"] if max_steps is None else max_steps
        m = m.cuda().eval()
        m.inference_batch([[5, 6]])  # creates the native handles while the variable is set
    finally:
        if old is None:
            del os.environ["TTS_RESIDENT"]
        else:
            os.environ["TTS_RESIDENT"] = old
    return m


def _ids(L):
    return weights_mod().synthetic_ids(L, 300 + L)


def _run(m, L, resident=True):
    out = m.inference_batch([_ids(L)])
    assert bool(m.last_timing["resident"]) == resident
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


@pytest.fixture(scope="module")
def flags():
    return golden_flags(golden("t2_fwdmask_L100"))  # synthesis configuration (synthesize.py:86)


@pytest.fixture(scope="module")
def model(flags):
    return _model(flags, True)


@pytest.mark.parametrize("L", LENGTHS)
def test_bit_identical_to_fixture(model, L):
    z = golden("resident_energy_partials")
    out = _run(model, L)
    T = int(out["frames"][0])
    assert T == int(z[f"L{L}_frames"][0])
    assert torch.equal(out["mel"][0, :T].cpu(), torch.from_numpy(z[f"L{L}_mel"]))
    assert torch.equal(out["align"][0, :T, :L].cpu(), torch.from_numpy(z[f"L{L}_align"]))
    assert torch.equal(out["stop"][0, :T].cpu(), torch.from_numpy(z[f"L{L}_stop"]))


def test_handle_reuse_across_step_parity(flags, model):
    """Runs that end on either step parity, then a full run, then a capped one again, on one
    handle: each equals the same run on a fresh handle."""
    L = 12
    caps = [5, 6, None, 5]
    fresh = {}
    for cap in (5, 6):
        fresh[cap] = _run(_model(flags, True, max_steps=cap), L)
        assert list(fresh[cap]["frames"]) == [cap]
    fresh[None] = _run(_model(flags, True), L)
    m = _model(flags, True)
    handle = m._native[0]
    for i, cap in enumerate(caps):
        # a run-time cap below the handles' capacity: assigning max_decoder_steps would re-create them
        m.set_step_cap(flags["max_decoder_steps"] if cap is None else cap)
        out = _run(m, L)
        assert m._native[0] is handle, "the model re-created its native handles"
        assert list(out["frames"]) == list(fresh[cap]["frames"]), f"call {i} (cap {cap})"
        for k in KEYS:
            assert torch.equal(out[k], fresh[cap][k]), f"call {i} (cap {cap}): {k}"


def test_resident_matches_multilaunch_L33(flags, model):
    L = 33
    a = _run(model, L)
    b = _run(_model(flags, False), L, resident=False)
    assert list(a["frames"]) == list(b["frames"])
    T = int(a["frames"][0])
    np.testing.assert_array_equal(a["align"][0, :T, :L].cpu().numpy().argmax(1),
                                  b["align"][0, :T, :L].cpu().numpy().argmax(1))
    d = rel_rms(a["mel"][0, :T].cpu().numpy(), b["mel"][0, :T].cpu().numpy())
    print(f"L={L}: frames {T}, mel rel rms resident vs multi-launch {d:.2e}")
    assert d < SAME_RTOL
