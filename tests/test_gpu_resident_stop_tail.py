"""GPU: the stop rule's tail in the resident batch-1 decoder (csrc/resident_decoder.hip).

The tail alpha[L-2] + alpha[L-1] (tacotron2.py:268) has one reader, the stop lane of each XCD's
stop CU.  In the synthesis configuration the attention CU publishes it as a granule after the
context; no gather waits for it, the stop lane loads it ahead of its h_dec gather and reads it in
step 11 (with a bounded wait of its own should it not be there yet).  The general form still
gathers its tail granule beside the context.  What can go wrong is a tail that is not this step's:
one left by the previous launch on the same handle, or by the other step parity, or none at a run
that the step cap ends.

The cases use the mask form (the t2_fwdmask flags) on one handle unless they say otherwise."""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle

pytestmark = pytest.mark.gpu

ORDER = [12, 2, 5, 3, 12]  # sentence lengths run in this order on one handle
KEYS = ("mel", "align", "stop")
SAME_RTOL = 1e-5  # resident vs multi-launch: the same fp32 step, different reduction orders (test_gpu_resident.py)


def _model(fl, env, max_steps=None):
    """A model whose native handles are created under the environment `env`."""
    t2 = load_pkg("tacotron2")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = t2.Tacotron2(130, 0, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                         forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                         forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"])
        m.decoder.max_decoder_steps = fl["max_decoder_steps"] if max_steps is None else max_steps
        m = m.cuda().eval()
        m.inference_batch([[5, 6]])  # creates the native handles while the variables are set
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return m


def _ids(L):
    return weights_mod().synthetic_ids(L, 300 + L)


def _run(m, L):
    out = m.inference_batch([_ids(L)])
    assert m.last_timing["resident"], "the resident decoder did not serve a batch-1 call"
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def _assert_same(a, b):
    assert list(a["frames"]) == list(b["frames"])
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def flags():
    return golden_flags(golden("t2_fwdmask_L100"))  # synthesis configuration (synthesize.py:86)


@pytest.fixture(scope="module")
def model(flags):
    return _model(flags, {"TTS_RESIDENT": "1"})


@pytest.fixture(scope="module")
def alone(flags):
    """Every length of this file on a fresh handle that has run nothing else (shared, not modified)."""
    res = {}
    for L in sorted(set(ORDER) | {4, 7}):
        res[L] = _run(_model(flags, {"TTS_RESIDENT": "1"}), L)
    return res


def test_alternating_lengths_equal_fresh_handle(model, alone):
    """Consecutive launches of different lengths on one handle: each equals the sentence run alone
    on a fresh handle (frames, mel, align, stop bit for bit)."""
    for i, L in enumerate(ORDER):
        out = _run(model, L)
        try:
            _assert_same(out, alone[L])
        except AssertionError as e:
            raise AssertionError(f"call {i} (L = {L}): {e}") from None


def _first_tail_step(align, L):
    """First step whose tail alpha[L-2] + alpha[L-1] exceeds 0.8 (fp32 sum; -1: none)."""
    a = np.asarray(align, np.float32)
    hit = np.nonzero((a[:, L - 2] + a[:, L - 1]) > np.float32(0.8))[0]
    return int(hit[0]) if hit.size else -1


@pytest.mark.parametrize("L", [2, 3, 4, 7])
def test_stop_step_against_oracle(alone, flags, L):
    """L - 2 and L - 1 both inside the window, and the window wrapping: the step at which the tail
    first exceeds 0.8 and the final frame count are the oracle's."""
    out = alone[L]
    ref = Tacotron2Oracle(weights_mod().tacotron2_weights(0), dtype=np.float32, **flags).inference(_ids(L))
    T = int(out["frames"][0])
    mine = _first_tail_step(out["align"][0, :T, :L].cpu().numpy(), L)
    want = _first_tail_step(ref["align"], L)
    print(f"L={L}: first tail step {mine} (oracle {want}), frames {T} (oracle {ref['mel'].shape[0]})")
    assert want >= 0, "the oracle's run never meets the tail condition: the case checks nothing"
    assert mine == want
    assert T == ref["mel"].shape[0]


@pytest.mark.parametrize("cap", [5, 6])
def test_step_cap_ends_the_run(flags, cap):
    """max_decoder_steps ends the run before the stop rule does (odd and even last-step parity):
    frames equal the cap, and the state left for the multi-launch path is what a multi-launch run
    of the same sentence leaves: a continued call (tts_decoder_run_continue) from either gives the
    same frames and the same mel to fp32 reduction-order noise."""
    L = 12
    res = _model(flags, {"TTS_RESIDENT": "1"}, max_steps=cap)
    ml = _model(flags, {"TTS_RESIDENT": "0"}, max_steps=cap)
    a = res.inference_batch([_ids(L)])
    assert res.last_timing["resident"]
    b = ml.inference_batch([_ids(L)])
    assert not ml.last_timing["resident"]
    assert list(a["frames"]) == [cap] and list(b["frames"]) == [cap]
    assert rel_rms(a["mel"][0].cpu().numpy(), b["mel"][0].cpu().numpy()) < SAME_RTOL
    # the same encoder outputs into both continued calls: only the carried decoder state differs
    enc = res.encode(torch.as_tensor(np.asarray(_ids(L)), dtype=torch.long)[None].cuda(), [L])
    a2 = res.inference_batch(None, enc=enc, lens=[L], _continue=True)
    assert res.last_timing["resident"]
    b2 = ml.inference_batch(None, enc=enc.clone(), lens=[L], _continue=True)
    assert not ml.last_timing["resident"]
    assert list(a2["frames"]) == [cap] and list(b2["frames"]) == [cap]
    d = rel_rms(a2["mel"][0].cpu().numpy(), b2["mel"][0].cpu().numpy())
    print(f"cap={cap}: continued-call mel rel rms {d:.2e}")
    assert d < SAME_RTOL
    np.testing.assert_array_equal(a2["align"][0, :, :L].cpu().numpy().argmax(1),
                                  b2["align"][0, :, :L].cpu().numpy().argmax(1))
    # and the continued call differs from a restart, so the comparison does see the carried state
    assert not torch.equal(a2["mel"], a["mel"])


def test_general_form_alternating_lengths():
    """The general attention form (the t2_nomask_L12 configuration), L = 12 alternated with L = 3 on
    one handle: each call equals the sentence run alone on a fresh handle."""
    fl = golden_flags(golden("t2_nomask_L12"))
    env = {"TTS_RESIDENT": "1", "TTS_RESIDENT_GEN": "1"}
    fresh = {L: _run(_model(fl, env), L) for L in (12, 3)}
    m = _model(fl, env)
    for i, L in enumerate([12, 3, 12, 3]):
        out = _run(m, L)
        try:
            _assert_same(out, fresh[L])
        except AssertionError as e:
            raise AssertionError(f"call {i} (L = {L}): {e}") from None
