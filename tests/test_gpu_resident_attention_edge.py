"""GPU: the resident batch-1 decoder's attention step and context hand-off (csrc/resident_decoder.hip,
synthesis configuration) at the sentence lengths where the mask's window logic can go wrong:
(n-2) mod L wraps, the 0.01-max position falls inside [n-1, n+2], the window clamps at L-1, the stop
rule's tail sees both L-2 and L-1 inside the window, and step 0 evaluates every position.

The fixture tests/golden/resident_attention_edge.npz holds the resident outputs (mel, align, stop,
frames) of the t2_fwdmask configuration for synthetic_ids(L, 300 + L), L in {2, 3, 4, 5, 6, 7, 12},
as computed by the build of commit bb261bf (the last one whose attention CU formed and published
all 512 context channels itself).  The attention step keeps every floating-point expression and
its order, so the outputs must stay equal bit for bit.  A compiler change may legitimately move a
bit; the fixture is then regenerated from a known-good build, not from the code under test."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 4, 5, 6, 7, 12]


@pytest.fixture(scope="module")
def flags():
    return golden_flags(golden("t2_fwdmask_L100"))  # synthesis configuration (synthesize.py:86)


@pytest.fixture(scope="module")
def model(flags, monkeypatch_module):
    monkeypatch_module.setenv("TTS_RESIDENT", "1")
    t2 = load_pkg("tacotron2")
    m = t2.Tacotron2(130, 0, r=1, attn_win=flags["attn_win"], attn_norm=flags["attn_norm"],
                     forward_attn=flags["forward_attn"], trans_agent=flags["trans_agent"],
                     forward_attn_mask=flags["forward_attn_mask"], location_attn=flags["location_attn"])
    m.decoder.max_decoder_steps = flags["max_decoder_steps"]
    m = m.cuda().eval()
    m.inference_batch([[5, 6]])  # creates the native handles while the variable is set
    return m


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def outputs(model):
    """One resident run per length, shared by the tests below (tensors are not modified)."""
    w = weights_mod()
    res = {}
    for L in LENGTHS:
        ids = w.synthetic_ids(L, 300 + L)
        out = model.inference_batch([ids])
        assert model.last_timing["resident"], "the resident decoder did not serve a batch-1 call"
        res[L] = (ids, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()})
    return res


@pytest.mark.parametrize("L", LENGTHS)
def test_bit_identical_to_fixture(outputs, L):
    z = golden("resident_attention_edge")
    _, out = outputs[L]
    T = int(out["frames"][0])
    assert T == int(z[f"L{L}_frames"][0])
    assert torch.equal(out["mel"][0, :T].cpu(), torch.from_numpy(z[f"L{L}_mel"]))
    assert torch.equal(out["align"][0, :T, :L].cpu(), torch.from_numpy(z[f"L{L}_align"]))
    assert torch.equal(out["stop"][0, :T].cpu(), torch.from_numpy(z[f"L{L}_stop"]))


@pytest.mark.parametrize("L", LENGTHS)
def test_against_oracle(outputs, flags, L):
    ids, out = outputs[L]
    ref = Tacotron2Oracle(weights_mod().tacotron2_weights(0), dtype=np.float32, **flags).inference(ids)
    T = int(out["frames"][0])
    assert T == ref["mel"].shape[0]  # exact frames
    np.testing.assert_array_equal(out["align"][0, :T, :L].cpu().numpy().argmax(1), ref["align"].argmax(1))
    np.testing.assert_array_equal(out["stop"][0, :T].cpu().numpy() > 0.5, np.asarray(ref["stop"]).reshape(-1)[:T] > 0.5)
    assert rel_rms(out["mel"][0, :T].cpu().numpy(), ref["mel"]) < 4e-6
    assert rel_rms(out["mel_post"][0, :T].cpu().numpy(), ref["mel_post"]) < 4e-6


@pytest.mark.parametrize("L", LENGTHS)
def test_consecutive_calls_identical(model, outputs, L):
    ids, first = outputs[L]
    again = model.inference_batch([ids])
    assert model.last_timing["resident"]
    assert list(again["frames"]) == list(first["frames"])
    for k in ("mel", "mel_post", "align", "stop"):
        assert torch.equal(again[k], first[k]), k
