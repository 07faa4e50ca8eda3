"""GPU parity of the resident batch decoder (csrc/resident_batch.hip): 2..12 sentences decoded in
one persistent launch per group of 4 with both LSTMs' weights held in registers, each sentence with
the reference's batch-1 semantics (Decoder.inference, layers/tacotron2.py:249-285).

Against the reference's own outputs (tests/golden/t2_*.npz, made by make_golden.py) in ragged
batches: frame counts, per-step attention argmax and stop decisions exact, mel / mel_post relative
RMS and alignments / stop max-abs at the model-half tolerance.  Sentences without a fixture come
from the numpy oracle (oracle/tacotron2_oracle.py, pinned on those fixtures) at the same flags.
Also: the path taken, groups of 4 (B = 8), the Synthesizer's 3000-step cap past the 2048-step tag
wrap, the multi-launch path on the same batch, and bitwise determinism.
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle

pytestmark = pytest.mark.gpu
MEL_RTOL = 4e-6   # model half: 10x the measured worst case (profiles/r05f_parity_report.jsonl)
ALIGN_ATOL = 4e-6
SAME_RTOL = 1e-5  # resident batch vs multi-launch: two fp32 reduction orders


def _model(fl, batch=True, max_batch=12):
    t2 = load_pkg("tacotron2")
    old = os.environ.get("TTS_RESIDENT_BATCH")
    os.environ["TTS_RESIDENT_BATCH"] = "1" if batch else "0"
    try:
        m = t2.Tacotron2(130, 0, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                         forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                         forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"],
                         max_batch=max_batch, max_len=256)
        m.decoder.max_decoder_steps = fl["max_decoder_steps"]
        m = m.cuda().eval()
        m.inference_batch([[5, 6], [7, 8, 9]])  # creates the native handles while the variable is set
    finally:
        if old is None:
            del os.environ["TTS_RESIDENT_BATCH"]
        else:
            os.environ["TTS_RESIDENT_BATCH"] = old
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
    np.testing.assert_array_equal(al.argmax(1), ref["align"].argmax(1))
    assert np.abs(al - ref["align"]).max() < ALIGN_ATOL
    st = out["stop"][b, :T].cpu().numpy()
    np.testing.assert_array_equal(st > 0.5, ref["stop"] > 0.5)
    assert np.abs(st - ref["stop"]).max() < ALIGN_ATOL
    assert rel_rms(out["mel"][b, :T].cpu().numpy(), ref["mel"]) < MEL_RTOL
    assert rel_rms(out["mel_post"][b, :T].cpu().numpy(), ref["mel_post"]) < MEL_RTOL


def _fix(name):
    z = golden(name)
    return dict(enc=z["enc"], mel=z["mel"], mel_post=z["mel_post"], align=z["align"], stop=z["stop"])


@pytest.mark.parametrize("cases", [
    ["t2_fwdmask_L100", "t2_fwdmask_L12"],
    ["t2_fwdmask_L12", "t2_fwdmask_L100", "t2_fwdmask_L40"],
    ["t2_fwdmask_L40", "t2_fwdmask_L12", "t2_fwdmask_L100", "t2_fwdmask_L12"],
    # two launches of 4 (groups), ragged
    ["t2_fwdmask_L12", "t2_fwdmask_L40", "t2_fwdmask_L100", "t2_fwdmask_L12",
     "t2_fwdmask_L100", "t2_fwdmask_L40", "t2_fwdmask_L12", "t2_fwdmask_L100"],
    # 4 + 1: the last launch holds one sentence (the NB = 2 kernel beside a padding sentence of
    # L = 0), one that none of the four before it equals
    ["t2_fwdmask_L12", "t2_fwdmask_L100", "t2_fwdmask_L100", "t2_fwdmask_L12", "t2_fwdmask_L40"],
    # 4 + 3
    ["t2_fwdmask_L100", "t2_fwdmask_L12", "t2_fwdmask_L40", "t2_fwdmask_L100",
     "t2_fwdmask_L40", "t2_fwdmask_L100", "t2_fwdmask_L12"],
])
def test_resident_batch_synthesis_configuration_vs_reference(cases):
    """synthesize.py's configuration (forward attention + eval mask, sigmoid) in ragged batches."""
    m = _model(golden_flags(golden(cases[0])))
    refs = [_fix(c) for c in cases]
    out = _run(m, [r["enc"] for r in refs])
    assert m.last_timing["resident_kind"] == 2, "the resident batch decoder did not serve this batch"
    for b, r in enumerate(refs):
        _check(out, b, r)


def test_resident_batch_mask_off_ragged_vs_reference_and_oracle():
    """Synthesizer.tts()'s configuration (mask off): the reference run t2_nomask_L12 (60-step cap)
    beside two sentences of other lengths from the oracle at the same flags."""
    z = golden("t2_nomask_L12")
    fl = golden_flags(z)
    m = _model(fl)
    o = Tacotron2Oracle(weights_mod().tacotron2_weights(0), dtype=np.float32, **fl)
    w = weights_mod()
    others = []
    for L, seed in ((30, 401), (7, 402)):
        ids = w.synthetic_ids(L, seed)
        enc = o.encoder(ids)
        mel, stop, align = o.decoder(enc)
        others.append(dict(enc=enc, mel=mel, mel_post=o.postnet(mel), align=align, stop=stop))
    refs = [others[0], _fix("t2_nomask_L12"), others[1]]
    out = _run(m, [r["enc"] for r in refs])
    assert m.last_timing["resident_kind"] == 2
    for b, r in enumerate(refs):
        _check(out, b, r)


@pytest.mark.parametrize("case", ["t2_nomask_L100", "t2_nomask_L100_cap3000"])
def test_resident_batch_mask_off_full_length(case):
    """The Synthesizer configuration over its full runs (1000 steps; 3000, the server's cap,
    server/synthesizer.py:66, past the 2048-step tag wrap), two sentences per launch."""
    z = golden(case)
    m = _model(golden_flags(z))
    out = _run(m, [z["enc"], z["enc"]])
    assert m.last_timing["resident_kind"] == 2
    for b in range(2):
        _check(out, b, _fix(case))


def test_resident_batch1_cap3000_vs_reference():
    """The batch-1 general resident form at the Synthesizer's 3000-step cap, pinned to the reference
    run itself (VERDICT r5 missing 3): frames, argmax and stop exact past the 2048-step tag wrap."""
    z = golden("t2_nomask_L100_cap3000")
    m = _model(golden_flags(z))
    out = _run(m, [z["enc"]])
    assert m.last_timing["resident_kind"] == 1
    _check(out, 0, _fix("t2_nomask_L100_cap3000"))


@pytest.mark.parametrize("mask", [True, False])
def test_resident_batch_vs_multilaunch(mask):
    """Ragged batch of 6 synthetic sentences (L 60..200): the resident batch decoder against the
    multi-launch path (frames, argmax, stop decisions exact; floats within two fp32 orders)."""
    fl = dict(golden_flags(golden("t2_fwdmask_L12")), forward_attn_mask=mask, max_decoder_steps=240)
    res, ml = _model(fl, True), _model(fl, False)
    w = weights_mod()
    lens = [60, 200, 97, 128, 75, 160]
    ids = [w.synthetic_ids(L, 500 + i) for i, L in enumerate(lens)]
    a = res.inference_batch(ids)
    assert res.last_timing["resident_kind"] == 2
    b = ml.inference_batch(ids)
    assert ml.last_timing["resident_kind"] == 0
    assert a["frames"] == b["frames"]
    for k in range(len(ids)):
        T, L = a["frames"][k], lens[k]
        aa, ab = a["align"][k, :T, :L].cpu().numpy(), b["align"][k, :T, :L].cpu().numpy()
        np.testing.assert_array_equal(aa.argmax(1), ab.argmax(1))
        assert np.abs(aa - ab).max() < SAME_RTOL
        sa, sb = a["stop"][k, :T].cpu().numpy(), b["stop"][k, :T].cpu().numpy()
        np.testing.assert_array_equal(sa > 0.5, sb > 0.5)
        for key in ("mel", "mel_post"):
            assert rel_rms(a[key][k, :T].cpu().numpy(), b[key][k, :T].cpu().numpy()) < SAME_RTOL, (k, key)


def test_resident_batch_deterministic():
    fl = golden_flags(golden("t2_fwdmask_L12"))
    m = _model(fl)
    refs = [_fix(c) for c in ("t2_fwdmask_L40", "t2_fwdmask_L12", "t2_fwdmask_L100")]
    a = _run(m, [r["enc"] for r in refs])
    b = _run(m, [r["enc"] for r in refs])
    assert a["frames"] == b["frames"]
    for k in ("mel", "mel_post", "align", "stop"):
        assert torch.equal(a[k], b[k]), k
