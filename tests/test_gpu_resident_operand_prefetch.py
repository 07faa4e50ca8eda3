"""GPU: the resident batch-1 decoder with the next step's attention operands (the entering encoder
row, P of the CU's four query dimensions at the 16 candidate slots) loaded by waves that do not
poll between B6 and the h_att gather, and handed to the polling waves through LDS
(csrc/resident_decoder.hip, synthesis configuration).  The values are the same bits whichever wave
loads them and no arithmetic changes, so nothing may move by a bit.

Every case compares mel, align, stop and frames with torch.equal against the fixture
tests/golden/resident_operand_prefetch.npz, written by tools/make_resident_operand_prefetch_golden.py
(which runs collect() below) on the build of commit 0c8ac1f, the last one with the loads ahead of
the h_att poll, not by the code under test.  Configuration t2_fwdmask, ids synthetic_ids(L, 300 + L).

- fresh_L2 / L3 / L5: the window wraps on every step, so the whole-window reload ahead of the
  h_att gather runs on every step and the LDS row slot is never used.
- fresh_L17 / L33: a candidate slot crosses the 16-slot boundary; slots past L read exactly 0.
- cap24_L256: the largest P offsets and row offsets (L = RES_LMAX), 24 steps.
- cap1 / cap2 at L = 12: the loads issued for a step that never runs must be harmless.
- cont_0 / 1 / 2: three consecutive segments (L = 12, 9, 12; 3, 2, 3 steps) through
  inference_truncated on one handle: the carried n; step 0's operands come from the carried state,
  not from LDS slots left by the previous launch.
- mixed_0 / 1: one handle, fresh full runs at L = 5, then L = 16 (a stale LDS slot across launches
  of different L).
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, weights_mod

pytestmark = pytest.mark.gpu

KEYS = ("mel", "align", "stop", "frames")
CASES = ("fresh_L2", "fresh_L3", "fresh_L5", "fresh_L17", "fresh_L33", "cap24_L256", "cap1_L12", "cap2_L12",
         "cont_0", "cont_1", "cont_2", "mixed_0", "mixed_1")
SEGMENTS = ((12, 3), (9, 2), (12, 3))  # (L, steps) of the continued run


def _model(fl):
    """A model whose native handles are created with the resident decoder on."""
    t2 = load_pkg("tacotron2")
    old = os.environ.get("TTS_RESIDENT")
    os.environ["TTS_RESIDENT"] = "1"
    try:
        m = t2.Tacotron2(130, 0, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                         forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                         forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"])
        m.decoder.max_decoder_steps = fl["max_decoder_steps"]
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


def _pack(m, L, mel, align, stop):
    assert bool(m.last_timing["resident"]), "the run left the resident path"
    T = int(m.last_lengths[0])
    return {"mel": mel[0, :T].cpu().numpy().copy(), "align": align[0, :T, :L].cpu().numpy().copy(),
            "stop": stop[0, :T].reshape(T).cpu().numpy().copy(), "frames": np.array([T], np.int64)}


def _batch(m, L):
    out = m.inference_batch([_ids(L)])
    return _pack(m, L, out["mel"], out["align"], out["stop"])


def _truncated(m, L):
    mel, _, align, stop = m.inference_truncated(torch.from_numpy(np.asarray(_ids(L)))[None])
    return _pack(m, L, mel, align, stop)


def collect(fl):
    """Every case's outputs, {case: {mel, align, stop, frames}} (numpy)."""
    full = fl["max_decoder_steps"]
    res = {}
    m = _model(fl)
    for L in (2, 3, 5, 17, 33):
        res[f"fresh_L{L}"] = _batch(m, L)
    for cap, L in ((24, 256), (1, 12), (2, 12)):
        m.set_step_cap(cap)  # a run-time cap below the handles' capacity keeps the handles
        res[f"cap{cap}_L{L}"] = _batch(m, L)
        assert list(res[f"cap{cap}_L{L}"]["frames"]) == [cap]
    m = _model(fl)
    handle = m._native[0]
    for i, (L, steps) in enumerate(SEGMENTS):
        m.set_step_cap(steps)
        res[f"cont_{i}"] = _truncated(m, L)
        assert list(res[f"cont_{i}"]["frames"]) == [steps]
    assert m._native[0] is handle, "the model re-created its native handles"
    m = _model(fl)
    handle = m._native[0]
    m.set_step_cap(full)
    res["mixed_0"] = _batch(m, 5)
    res["mixed_1"] = _batch(m, 16)
    assert m._native[0] is handle, "the model re-created its native handles"
    return res


@pytest.fixture(scope="module")
def results():
    return collect(golden_flags(golden("t2_fwdmask_L100")))  # synthesis configuration (synthesize.py:86)


@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_fixture(results, case):
    z = golden("resident_operand_prefetch")
    got = results[case]
    assert int(got["frames"][0]) == int(z[f"{case}_frames"][0])
    for k in KEYS:
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(z[f"{case}_{k}"])), f"{case}: {k}"


def test_cases_differ_where_the_state_differs():
    """The fixture itself: a continued segment is not the fresh run of the same text (the carried
    state and n reach step 0), a capped run is the head of a longer one, the fresh run on the mixed
    handle equals the plain fresh run, and the alignment rows of L = 17, 33 and 256 reach past the
    16-slot boundary."""
    z = golden("resident_operand_prefetch")
    assert not np.array_equal(z["cont_2_mel"], z["cont_0_mel"])
    assert not np.array_equal(z["cont_2_align"], z["cont_0_align"])
    for k in ("mel", "align", "stop"):
        np.testing.assert_array_equal(z[f"cap1_L12_{k}"], z[f"cap2_L12_{k}"][:1])
        np.testing.assert_array_equal(z[f"mixed_0_{k}"], z[f"fresh_L5_{k}"])
    assert not np.array_equal(z["mixed_1_mel"][:32], z["mixed_0_mel"])
    for case, L in (("fresh_L17", 17), ("fresh_L33", 33), ("cap24_L256", 256)):
        a = z[f"{case}_align"]
        assert a.shape[1] == L and (a >= 0).all()
    assert z["fresh_L33_align"][:, 16:].max() > 0.5  # the window crosses position 16
