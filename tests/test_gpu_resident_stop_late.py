"""GPU: the resident batch-1 decoder with step t's stop row and rule moved into step t+1 (the
stop CU forms them behind its prenet-2 row) and the continue check moved to the energy gather
(csrc/resident_decoder.hip, synthesis configuration).  The ending step now runs from P1 to A2
for a step that does not exist: it writes the last real step's stop value and mel row, updates
the attention LSTM's cell, and publishes h_att and energy partials under its own tags.  The
kernel restores (c_att, h_att) from the values it kept; no arithmetic changes, so nothing may
move by a bit.

Every case compares the frame count, n_steps, the handle's count of steps run, the last 8 rows
of mel / align / stop as raw values and zlib.crc32 of the full arrays' bytes with torch.equal
against the fixture tests/golden/resident_stop_late.npz, written by
tools/make_resident_stop_late_golden.py (which runs collect() below) on the build of commit
450aa7f, the last one with the rule in step 11 and the check behind B1, not by the code under
test.  Configuration t2_fwdmask, ids synthetic_ids(L, 300 + L).

- wrap_cap2047 / 2048 / 2049 (L = 12, handles created for 2049 steps): caps on both sides of the
  tags' 2048-step wrap.  With the test weights the rule stops an L = 12 sentence after 2 L + 22 =
  46 steps, so these runs end by the rule, not at the cap: they pin the outputs under the three
  caps, and the wrap itself (the parent's own tag expression, reused) is not reached by them.
- seg_0 / 1 / 2 / 3: four segments of one step each through inference_truncated on one handle
  (L = 2, 2, 5, 5).  Each ending step is step 1, right behind the full-evaluation step 0, with the
  whole window reloaded; a segment's output witnesses the (c_att, h_att) the one before restored.
- stopfresh_0 / 1: one handle, a natural stop at L = 3, then a fresh run at L = 33: the first
  run's ending step published h_att and partial granules under its own salt.
- capfull_L256: L = 256 with set_step_cap at the handle's capacity (the fixture flags'
  max_decoder_steps): the largest offsets; the rule stops it after 2 L + 22 = 534 steps.
"""
import zlib

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags
from test_gpu_resident_stop_deferred import _batch, _model, _truncated

pytestmark = pytest.mark.gpu

KEYS = ("frames", "n_steps", "steps_run", "mel_tail", "align_tail", "stop_tail", "crc")
CASES = ("wrap_cap2047", "wrap_cap2048", "wrap_cap2049", "seg_0", "seg_1", "seg_2", "seg_3",
         "stopfresh_0", "stopfresh_1", "capfull_L256")
WRAP_CAPS = (2047, 2048, 2049)
SEGMENTS = ((2, 1), (2, 1), (5, 1), (5, 1))  # (L, steps) of the continued run
TAIL = 8


def _digest(d):
    """What the fixture keeps of one run: counts, the last rows raw, crc32 of the whole arrays."""
    crc = [zlib.crc32(np.ascontiguousarray(d[k]).tobytes()) for k in ("mel", "align", "stop")]
    return {"frames": d["frames"], "n_steps": d["n_steps"], "steps_run": d["steps_run"],
            "mel_tail": d["mel"][-TAIL:].copy(), "align_tail": d["align"][-TAIL:].copy(),
            "stop_tail": d["stop"][-TAIL:].copy(), "crc": np.array(crc, np.int64)}


def collect(fl):
    """Every case's digest, {case: {frames, n_steps, steps_run, *_tail, crc}} (numpy)."""
    full = fl["max_decoder_steps"]
    res = {}
    m = _model(dict(fl, max_decoder_steps=max(WRAP_CAPS)))
    handle = m._native[0]
    for cap in WRAP_CAPS:
        m.set_step_cap(cap)
        res[f"wrap_cap{cap}"] = _digest(_batch(m, 12))
    assert m._native[0] is handle, "the model re-created its native handles"
    m = _model(fl)
    handle = m._native[0]
    for i, (L, steps) in enumerate(SEGMENTS):
        m.set_step_cap(steps)
        res[f"seg_{i}"] = _digest(_truncated(m, L))
        assert list(res[f"seg_{i}"]["frames"]) == [steps]
    assert m._native[0] is handle, "the model re-created its native handles"
    m = _model(fl)
    handle = m._native[0]
    m.set_step_cap(full)
    res["stopfresh_0"] = _digest(_batch(m, 3))
    res["stopfresh_1"] = _digest(_batch(m, 33))
    res["capfull_L256"] = _digest(_batch(m, 256))
    assert m._native[0] is handle, "the model re-created its native handles"
    return res


@pytest.fixture(scope="module")
def results():
    return collect(golden_flags(golden("t2_fwdmask_L100")))  # synthesis configuration (synthesize.py:86)


@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_fixture(results, case):
    z = golden("resident_stop_late")
    got = results[case]
    assert int(got["frames"][0]) == int(z[f"{case}_frames"][0])
    for k in KEYS:
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(z[f"{case}_{k}"])), f"{case}: {k}"


def test_fixture_cases_differ_where_the_state_differs():
    """The fixture itself: a segment behind the first is not the first (the carried state reaches
    its step 0), the runs of the reused handle equal the earlier fixture's fresh runs, the
    natural stops come 21 steps behind 2 L, and nothing is all zeros."""
    z = golden("resident_stop_late")
    old = golden("resident_stop_deferred")
    assert not np.array_equal(z["seg_1_mel_tail"], z["seg_0_mel_tail"])
    assert not np.array_equal(z["seg_3_mel_tail"], z["seg_2_mel_tail"])
    for case, ref in (("stopfresh_0", "fresh_L3"), ("stopfresh_1", "fresh_L33")):
        for k in ("mel", "align", "stop"):
            np.testing.assert_array_equal(z[f"{case}_{k}_tail"], old[f"{ref}_{k}"][-TAIL:])
    for case, L in (("wrap_cap2047", 12), ("wrap_cap2048", 12), ("wrap_cap2049", 12), ("stopfresh_0", 3),
                    ("stopfresh_1", 33), ("capfull_L256", 256)):
        assert int(z[f"{case}_frames"][0]) == 2 * L + 22, case
    for case in CASES:
        assert np.abs(z[f"{case}_mel_tail"]).max() > 0 and z[f"{case}_stop_tail"].max() > 0, case
        assert int(z[f"{case}_n_steps"][0]) == int(z[f"{case}_frames"][0]) > 0, case
        assert int(z[f"{case}_steps_run"][0]) > 0, case
        assert np.allclose(z[f"{case}_align_tail"].sum(1), 1.0, atol=1e-4), case
