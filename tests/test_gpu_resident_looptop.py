"""GPU: the resident batch-1 decoder with both LSTMs' recurrent partials moved off the loop top
(csrc/resident_decoder.hip, synthesis configuration).  The attention-LSTM partial over
[ctx_t | h_att_t] is formed inside step t's h_dec wait and carried to step t+1 (step 0's ahead of
the loop, from the initial or the carried state); the decoder-LSTM partial over h_dec_{t-1} inside
step t's h_att wait.  Chunk order, accumulator parity and the final adds are those of the loop-top
form, so nothing may move by a bit.

Every case compares mel, align, stop and frames with torch.equal against the fixture
tests/golden/resident_looptop.npz, written by tools/make_resident_looptop_golden.py (which runs
collect() below) on the build of commit af5c52d, the last one with the partials at the loop top,
not by the code under test.  Configuration t2_fwdmask, ids synthetic_ids(L, 300 + L).

- fresh_L2 / L5 / L16: fresh runs (at L = 2 the window wraps on every step).
- cap1 / cap2 / cap3 at L = 12: with cap 1 the loop ends after step 0, so the partial formed ahead
  of the loop is the only one used and the one formed in that step's h_dec wait is dropped; caps
  2 and 3 end on either granule parity.
- cont_0 / 1 / 2: three consecutive segments (L = 12, 9, 12; 3, 2, 3 steps) through
  inference_truncated on one handle: step 0 of segments 1 and 2 starts from the carried nonzero h,
  c and context (a partial formed ahead of the loop from the wrong state slot, or a decoder
  partial read after step 0's full evaluation has reused xh_dec as scratch, shows here).  Every
  segment must have run on the resident path.
- mixed_0 / 1 / 2: one handle, a fresh full run (L = 5), a continued 3-step run (L = 12), a fresh
  full run (L = 16).
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, weights_mod

pytestmark = pytest.mark.gpu

KEYS = ("mel", "align", "stop", "frames")
CASES = ("fresh_L2", "fresh_L5", "fresh_L16", "cap1_L12", "cap2_L12", "cap3_L12",
         "cont_0", "cont_1", "cont_2", "mixed_0", "mixed_1", "mixed_2")
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


def _batch(m, L, cont=False):
    out = m.inference_batch([_ids(L)], _continue=cont)
    return _pack(m, L, out["mel"], out["align"], out["stop"])


def _truncated(m, L):
    mel, _, align, stop = m.inference_truncated(torch.from_numpy(np.asarray(_ids(L)))[None])
    return _pack(m, L, mel, align, stop)


def collect(fl):
    """Every case's outputs, {case: {mel, align, stop, frames}} (numpy)."""
    full = fl["max_decoder_steps"]
    res = {}
    m = _model(fl)
    for L in (2, 5, 16):
        res[f"fresh_L{L}"] = _batch(m, L)
    for cap in (1, 2, 3):
        m.set_step_cap(cap)  # a run-time cap below the handles' capacity keeps the handles
        res[f"cap{cap}_L12"] = _batch(m, 12)
        assert list(res[f"cap{cap}_L12"]["frames"]) == [cap]
    m = _model(fl)
    handle = m._native[0]
    for i, (L, steps) in enumerate(SEGMENTS):
        m.set_step_cap(steps)
        res[f"cont_{i}"] = _truncated(m, L)
        assert list(res[f"cont_{i}"]["frames"]) == [steps]
    assert m._native[0] is handle, "the model re-created its native handles"
    m = _model(fl)
    handle = m._native[0]
    res["mixed_0"] = _batch(m, 5)
    m.set_step_cap(3)
    res["mixed_1"] = _batch(m, 12, cont=True)
    m.set_step_cap(full)
    res["mixed_2"] = _batch(m, 16)
    assert m._native[0] is handle, "the model re-created its native handles"
    return res


@pytest.fixture(scope="module")
def results():
    return collect(golden_flags(golden("t2_fwdmask_L100")))  # synthesis configuration (synthesize.py:86)


@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_fixture(results, case):
    z = golden("resident_looptop")
    got = results[case]
    assert int(got["frames"][0]) == int(z[f"{case}_frames"][0])
    for k in KEYS:
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(z[f"{case}_{k}"])), f"{case}: {k}"


def test_cases_differ_where_the_state_differs():
    """The fixture itself: a continued segment is not the fresh run of the same text (the carried
    state reaches step 0), and the fresh runs on the mixed handle equal the plain fresh runs."""
    z = golden("resident_looptop")
    assert not np.array_equal(z["cont_2_mel"], z["cap3_L12_mel"])
    assert not np.array_equal(z["mixed_1_mel"], z["cap3_L12_mel"])
    for k in KEYS:
        np.testing.assert_array_equal(z[f"mixed_0_{k}"], z[f"fresh_L5_{k}"])
        np.testing.assert_array_equal(z[f"mixed_2_{k}"], z[f"fresh_L16_{k}"])
