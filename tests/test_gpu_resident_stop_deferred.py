"""GPU: the resident batch-1 decoder with the continue check taken off the prenet-1 edge
(csrc/resident_decoder.hip, synthesis configuration): wave 2 sweeps the previous step's continue
flag behind its prenet-2 row and the loop ends after B1, so the ending step runs the part between
P1 and B1 once for a step that does not exist; the stop CU forms the stop row in a pass of its own
behind its prenet-1 row.  No arithmetic changes, so nothing may move by a bit, and the extra
half-step may leave nothing behind.

Every case compares mel, align, stop, the frame count and the step counts (n_steps as
inference_batch returns it, and the handle's count of steps run) with torch.equal against the
fixture tests/golden/resident_stop_deferred.npz, written by
tools/make_resident_stop_deferred_golden.py (which runs collect() below) on the build of commit
3550ced, the last one with the flag polled ahead of P1, not by the code under test.  Configuration
t2_fwdmask, ids synthetic_ids(L, 300 + L).

- fresh_L2 / L3 / L5 / L17 / L33: to the natural stop (the rule fires after t > 2 L, then 21 steps);
  L <= 5 reloads the whole window on every step.
- cap1 / cap2 at L = 12: the ending step is step 1 or 2, right behind step 0's special cases.
- cap24_L256: the largest offsets (L = RES_LMAX), 24 steps.
- cont_0 / 1 / 2 / 3: consecutive segments (L = 12, 9, 12, 9; 3, 2, 3, 2 steps) through
  inference_truncated on one handle.  The handle's state is not readable from Python; the state a
  segment leaves (h, c of both LSTMs, the context, the prenet-1 vector of the next step) is step 0's
  input of the next segment, so each segment's outputs witness the state carried out of the one
  before, and the fourth segment is there to witness the third's.
- mixed_0 / 1: one handle, fresh full runs at L = 5, then L = 16 (stale LDS and granules across
  launches).
- twice_0 / 1: the same L = 17 sentence twice on one handle: the first run's ending step published
  prenet-2 rows under another salt.
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, weights_mod

pytestmark = pytest.mark.gpu

KEYS = ("mel", "align", "stop", "frames", "n_steps", "steps_run")
CASES = ("fresh_L2", "fresh_L3", "fresh_L5", "fresh_L17", "fresh_L33", "cap1_L12", "cap2_L12", "cap24_L256",
         "cont_0", "cont_1", "cont_2", "cont_3", "mixed_0", "mixed_1", "twice_0", "twice_1")
SEGMENTS = ((12, 3), (9, 2), (12, 3), (9, 2))  # (L, steps) of the continued run


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


def _pack(m, L, mel, align, stop, steps):
    assert bool(m.last_timing["resident"]), "the run left the resident path"
    T = int(m.last_lengths[0])
    return {"mel": mel[0, :T].cpu().numpy().copy(), "align": align[0, :T, :L].cpu().numpy().copy(),
            "stop": stop[0, :T].reshape(T).cpu().numpy().copy(), "frames": np.array([T], np.int64),
            "n_steps": np.array([steps], np.int64),
            "steps_run": np.array([m.last_timing["decoder_steps_run"]], np.int64)}


def _batch(m, L):
    out = m.inference_batch([_ids(L)])
    return _pack(m, L, out["mel"], out["align"], out["stop"], out["steps"][0])


def _truncated(m, L):
    mel, _, align, stop = m.inference_truncated(torch.from_numpy(np.asarray(_ids(L)))[None])
    return _pack(m, L, mel, align, stop, int(m.last_lengths[0]) // m.n_frames_per_step)


def collect(fl):
    """Every case's outputs, {case: {mel, align, stop, frames, n_steps, steps_run}} (numpy)."""
    full = fl["max_decoder_steps"]
    res = {}
    m = _model(fl)
    for L in (2, 3, 5, 17, 33):
        res[f"fresh_L{L}"] = _batch(m, L)
    for cap, L in ((1, 12), (2, 12), (24, 256)):
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
    m = _model(fl)
    handle = m._native[0]
    m.set_step_cap(full)
    res["twice_0"] = _batch(m, 17)
    res["twice_1"] = _batch(m, 17)
    assert m._native[0] is handle, "the model re-created its native handles"
    return res


@pytest.fixture(scope="module")
def results():
    return collect(golden_flags(golden("t2_fwdmask_L100")))  # synthesis configuration (synthesize.py:86)


@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_fixture(results, case):
    z = golden("resident_stop_deferred")
    got = results[case]
    assert int(got["frames"][0]) == int(z[f"{case}_frames"][0])
    for k in KEYS:
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(z[f"{case}_{k}"])), f"{case}: {k}"


def test_second_run_equals_the_first(results):
    for k in KEYS:
        assert torch.equal(torch.from_numpy(results["twice_0"][k]), torch.from_numpy(results["twice_1"][k])), k


def test_cases_differ_where_the_state_differs():
    """The fixture itself: a continued segment is not the fresh run of the same text (the carried
    state reaches step 0, for every segment behind the first), a capped run is the head of a
    longer one, the fresh runs on the mixed and the twice-used handle equal the plain fresh runs,
    the natural stops come 21 steps behind 2 L at the earliest, and nothing is all zeros."""
    z = golden("resident_stop_deferred")
    assert not np.array_equal(z["cont_2_mel"], z["cont_0_mel"])
    assert not np.array_equal(z["cont_2_align"], z["cont_0_align"])
    assert not np.array_equal(z["cont_3_mel"], z["cont_1_mel"])
    for k in ("mel", "align", "stop"):
        np.testing.assert_array_equal(z[f"cap1_L12_{k}"], z[f"cap2_L12_{k}"][:1])
        np.testing.assert_array_equal(z[f"mixed_0_{k}"], z[f"fresh_L5_{k}"])
        np.testing.assert_array_equal(z[f"twice_0_{k}"], z[f"fresh_L17_{k}"])
        np.testing.assert_array_equal(z[f"twice_1_{k}"], z[f"fresh_L17_{k}"])
    assert not np.array_equal(z["mixed_1_mel"][:32], z["mixed_0_mel"][:32])
    cap = golden_flags(golden("t2_fwdmask_L100"))["max_decoder_steps"]
    for L in (2, 3, 5, 17, 33):
        T = int(z[f"fresh_L{L}_frames"][0])
        assert T == int(z[f"fresh_L{L}_n_steps"][0]) == z[f"fresh_L{L}_mel"].shape[0]
        assert 2 * L + 21 < T < cap, (L, T)  # the rule's stop, not the step cap
    for case in CASES:
        assert np.abs(z[f"{case}_mel"]).max() > 0 and z[f"{case}_stop"].max() > 0, case
        assert int(z[f"{case}_n_steps"][0]) == int(z[f"{case}_frames"][0]) > 0, case
        assert np.allclose(z[f"{case}_align"].sum(1), 1.0, atol=1e-4), case
