"""GPU parity of the multi-launch batched decoder step (csrc/decoder_api.hip: enqueue_step; the
launches sgemm_frag* / frag16 of csrc/sgemm.hip: launch_role, query_energy and attention_fm), which
serves every batch above 8 sentences: EVERY sentence of the batch against the reference, at batch
sizes on the edges of the 16-sentence GEMM tiles.

Batches are drawn from a pool of ten reference runs (tests/golden/pool_fwdmask.npz, made by
make_golden.py "pool": L = 2..40 at batch 1, synthesize.py's configuration: forward attention with
the eval mask).  Slot b of a batch of B holds pool sentence perm_B[b % 10], perm_B a fixed
permutation seeded by B: every tile mixes lengths, its sentences finish at different steps
(2L + 22 frames), and a sentence sits in another tile row at every B.  The decoder gets the
reference's own encoder outputs, so it is the only thing under test.

B = 9 is the first batch past the resident batch decoder (row-major GEMM inputs up to 16); from 17
the GEMMs read fragment mirrors whose stride comes from the handle's max_batch (ntf tiles), not from
B.  B = 16 / 32 / 48 / 64 fill their tiles, 17 / 33 / 49 end in a tile of one sentence, and 33..48
(3 tiles) run the 4-tile kernel with an empty tile.  max_batch = B (17, 33) gives ntf = 2 and 3.

The check is test_gpu_parity.py's _check_decoder: frame count, per-step attention argmax and stop
decisions exact, alignments / stop max-abs < 4e-6, mel / mel_post relative RMS < 4e-6 (10x the
worst case of profiles/r05f_parity_report.jsonl).  The worst measured value per case is kept in
profiles/multilaunch_batch_parity.jsonl, written when TTS_PARITY_REPORT names the file:

    TTS_PARITY_REPORT=profiles/multilaunch_batch_parity.jsonl pytest tests/test_gpu_multilaunch_batch.py
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle

pytestmark = pytest.mark.gpu
MEL_RTOL = 4e-6   # model half: 10x the measured worst case (profiles/r05f_parity_report.jsonl)
ALIGN_ATOL = 4e-6
KEYS = ("enc", "mel", "mel_post", "align", "stop")
_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("TTS_PARITY_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            for rec in _REPORT:
                f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def pool():
    """{L: reference run} of the pool fixture, and its flags."""
    z = golden("pool_fwdmask")
    lengths = [int(L) for L in z["lengths"]]
    assert len(lengths) == 10
    return {L: {k: z[f"{k}_L{L}"] for k in KEYS} for L in lengths}, golden_flags(z)


@pytest.fixture(scope="module")
def pool_mask_off(pool):
    """Synthesizer.tts()'s configuration (mask off, which runs to the cap under these weights) at a
    40-step cap: the pool's L = 5, 13, 24 and 40 encoder outputs through the fp64 oracle (pinned to
    the reference in this configuration by t2_nomask_L12), computed once."""
    sents, fl = pool
    fl = dict(fl, forward_attn_mask=False, max_decoder_steps=40)
    o = Tacotron2Oracle(weights_mod().tacotron2_weights(0), dtype=np.float64, **fl)
    refs = {}
    for L in (5, 13, 24, 40):
        enc = sents[L]["enc"]
        mel, stop, align = o.decoder(enc)
        refs[L] = dict(enc=enc, mel=mel, mel_post=o.postnet(mel), align=align, stop=stop)
    return refs, fl


def _model(fl, max_batch):
    t2 = load_pkg("tacotron2")
    m = t2.Tacotron2(130, 0, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                     forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                     forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"],
                     max_batch=max_batch)
    m.decoder.max_decoder_steps = fl["max_decoder_steps"]
    return m.cuda().eval()


@pytest.fixture(scope="module")
def model64(pool):
    """One max_batch = 64 handle (ntf = 4) for the whole module: the cases run on whatever the
    previous ones left in its mirrors, done flags and per-slot state."""
    return _model(pool[1], 64)


def _batch(sents, B):
    """The B reference runs of a batch: slot b holds sentence perm[b % n] of the (length-sorted) pool."""
    Ls = sorted(sents)
    perm = np.random.Generator(np.random.PCG64(B)).permutation(len(Ls))
    return [sents[Ls[perm[b % len(Ls)]]] for b in range(B)]


def _run(m, refs):
    lens = [r["enc"].shape[0] for r in refs]
    enc = torch.zeros(len(refs), max(lens), 512)
    for b, r in enumerate(refs):
        enc[b, :lens[b]] = torch.from_numpy(r["enc"])
    out = m.inference_batch(None, enc=enc.cuda(), lens=lens)
    assert m.last_timing["resident_kind"] == 0, "the multi-launch step did not serve this batch"
    return out


def _check_all(out, refs, case):
    """Every slot of the batch against its reference run (test_gpu_parity.py: _check_decoder); the
    worst value of each float quantity over the batch goes to the report before anything is asserted."""
    B = len(refs)
    rec = dict(case=case, B=B, frames_exact=True, argmax_exact=True, stop_exact=True,
               align_maxabs=0.0, stop_maxabs=0.0, mel_rel=0.0, mel_post_rel=0.0)
    bad = []
    mel, mel_post = out["mel"].cpu().numpy(), out["mel_post"].cpu().numpy()
    align, stop = out["align"].cpu().numpy(), out["stop"].cpu().numpy()
    for b, r in enumerate(refs):
        T, L = out["frames"][b], r["enc"].shape[0]
        if T != r["mel"].shape[0]:
            rec["frames_exact"] = False
            bad.append(f"slot {b} (L={L}): {T} frames, reference {r['mel'].shape[0]}")
            continue
        al, st = align[b, :T, :L], stop[b, :T]
        if not np.array_equal(al.argmax(1), r["align"].argmax(1)):
            rec["argmax_exact"] = False
            bad.append(f"slot {b} (L={L}): attention argmax differs")
        if not np.array_equal(st > 0.5, r["stop"] > 0.5):
            rec["stop_exact"] = False
            bad.append(f"slot {b} (L={L}): stop decisions differ")
        vals = dict(align_maxabs=float(np.abs(al - r["align"]).max()), stop_maxabs=float(np.abs(st - r["stop"]).max()),
                    mel_rel=rel_rms(mel[b, :T], r["mel"]), mel_post_rel=rel_rms(mel_post[b, :T], r["mel_post"]))
        for k, v in vals.items():
            rec[k] = max(rec[k], v)
            if not v < (MEL_RTOL if k.startswith("mel") else ALIGN_ATOL):
                bad.append(f"slot {b} (L={L}): {k} = {v:.3e}")
    rec.update({k: float(f"{rec[k]:.4g}") for k in ("align_maxabs", "stop_maxabs", "mel_rel", "mel_post_rel")})
    print(json.dumps(rec))
    _REPORT.append(rec)
    assert not bad, bad


@pytest.mark.parametrize("B", [9, 16, 17, 32, 33, 48, 49, 64])
def test_every_sentence_vs_reference(pool, model64, B):
    """The headline configuration (query_energy + attention_fm) on a max_batch = 64 handle at every
    tile edge: row-major GEMM inputs (9, 16), fragment mirrors with full last tiles (32, 48, 64),
    with a one-sentence last tile (17, 33, 49), and three tiles on the four-tile kernel (33, 48)."""
    refs = _batch(pool[0], B)
    _check_all(_run(model64, refs), refs, "every_sentence")


@pytest.mark.parametrize("B", [17, 33])
def test_handle_sized_to_batch(pool, B):
    """max_batch = B: the mirrors' tile stride ntf equals the batch's own tile count (2 and 3, not 4)."""
    refs = _batch(pool[0], B)
    _check_all(_run(_model(pool[1], B), refs), refs, "handle_sized_to_batch")


def test_padding_untouched(pool, model64):
    """B = 33: inference_batch zero-fills mel, stop and align before the run, and the decoder owes
    sentence b only its own T_b steps and L_b positions: everything past them stays exactly zero
    (tts_decoder_run: zero up to the batch's longest run, untouched beyond it).  A sentence that
    keeps writing after `done`, a write into a neighbour's slot, or rows of an earlier run left in
    the handle's histories (model64 has run longer sentences in these slots) show here.

    mel_post: tts_postnet_run's contract is that frames past T_b are not computed and its rows
    t >= T_b are left untouched (postnet.hip: postnet_run_dev, conv1d.hip's epilogues); it promises
    no zeros of its own.  inference_batch hands it a zero-filled buffer, so untouched means zero
    here, and that is what is asserted."""
    _run(model64, _batch(pool[0], 64))  # another permutation: a longer sentence in 13 of the 33 slots
    refs = _batch(pool[0], 33)
    out = _run(model64, refs)
    for b, r in enumerate(refs):
        T, L = out["frames"][b], r["enc"].shape[0]
        assert T == r["mel"].shape[0]
        for k in ("mel", "stop", "align", "mel_post"):
            assert not out[k][b, T:].any(), f"slot {b} (L={L}, T={T}): {k} written past its last step"
        assert not out["align"][b, :T, L:].any(), f"slot {b} (L={L}): alignment past the sentence's length"
    assert max(out["frames"]) == 102 and min(out["frames"]) == 26  # the padding is there to check


def test_small_batch_after_large_on_one_handle(pool):
    """B = 64, then 17, then 33 on one max_batch = 64 handle.  The small batches give the reference's
    results and, bit for bit, what a fresh handle gives for the same batch: the same kernels on the
    same inputs, unless mirrors, done flags or slot state of the larger run leak."""
    sents, fl = pool
    first = {B: _run(_model(fl, 64), _batch(sents, B)) for B in (17, 33)}
    m = _model(fl, 64)
    for B in (64, 17, 33):
        refs = _batch(sents, B)
        out = _run(m, refs)
        _check_all(out, refs, "after_B64" if B != 64 else "before_small")
        if B in first:
            assert out["frames"] == first[B]["frames"]
            for k in ("mel", "mel_post", "align", "stop"):
                assert torch.equal(out[k], first[B][k]), (B, k)


def test_deterministic(pool, model64):
    """B = 49 twice on one handle: all four outputs bitwise equal."""
    refs = _batch(pool[0], 49)
    a, b = _run(model64, refs), _run(model64, refs)
    assert a["frames"] == b["frames"]
    for k in ("mel", "mel_post", "align", "stop"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("B", [17, 64])
def test_mask_off_every_sentence(pool_mask_off, B):
    """Synthesizer.tts()'s configuration (mask off) at a 40-step cap: the general attention launch
    (attention.hip) through the fragment mirrors, every sentence against the oracle.  Without the
    mask these weights give every exit of the stop rule in one batch: L = 5 stops by itself (32
    frames), L = 24 and 40 end at the cap (40), L = 13 has every stop flag set near the cap and runs
    past it (54; layers/tacotron2.py:271-277)."""
    sents, fl = pool_mask_off
    assert {L: r["mel"].shape[0] for L, r in sents.items()} == {5: 32, 13: 54, 24: 40, 40: 40}
    refs = _batch(sents, B)
    _check_all(_run(_model(fl, 64), refs), refs, "mask_off")
