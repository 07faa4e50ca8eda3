"""Case table, inputs, float64 reference and comparison of the resident TacotronGST decoder's contract tests
(tests/test_gpu_tacotron_resident_contract.py on the device, tests/test_tacotron_resident_util_cpu.py for the
cases and the comparator themselves, tools/tacotron_resident_report.py for the record).  Imports without a GPU.

The kernel (csrc/tacotron_resident.hip) cuts a sentence's encoder positions into 8 slices of 32, the batch
into groups of 4 sentences, and the mel rows into m0 = r + 32 w, m1 = m0 + 256; the cases put a length, a
batch size or an (r, memory_size) on each side of every one of those cuts.

Inputs: weights.tacotron_gst_weights(0, r, memory_size); a sentence of length L is the float64 oracle encoder's
output for weights.synthetic_ids(L, 900 + L), rounded to float32 (the encoder weights do not depend on r or
memory_size: one stream per key).  A tail case multiplies the sentence's last encoder row by a factor c, which
makes the alignment-tail stop rule fire (alpha[L-1] > 0.6) where the unmodified sentence only ends at the step
cap.  The device gets the rows through inference_batch(None, enc=..., lens=..., postnet=False), the reference is
TacotronOracle(dtype=float64).decoder() on the same float32 values: the decoder alone.

Tolerances are tests/test_gpu_tacotron.py's ATOL / RTOL.
"""
import collections
import functools

import numpy as np

from conftest import golden, golden_flags, rel_rms, weights_mod

ATOL = 4e-6          # alignment rows, stop values: max-abs
RTOL = 4e-6          # mel: relative RMS
TIE_GAP = 2 * ATOL   # the argmax of a step is compared where the oracle's top two are further apart
SKIP_CAP = 0.03      # ... and at most this share of a sentence's steps may be left out
MARGIN = 1e-3        # every decision of a case keeps this distance from 0.6 in the oracle (250 x ATOL)
PPC = 32             # TR_PPC: encoder positions per attention slice

Sent = collections.namedtuple("Sent", "L c")   # c: factor on the last encoder row (1.0: unmodified)


def S(L, c=1.0):
    return Sent(int(L), float(c))


EDGE_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97)
# tail cases: L -> c, found on the CPU with the float64 oracle (test_tail_cases_stop_by_the_tail_rule holds the
# steps); the tail sits at local index 31, 0, 31, 0, 0 of slices 0, 1, 1, 2, 4
TAIL_FACTOR = {32: 8.0, 33: 8.0, 64: 8.0, 65: 8.0, 129: 32.0}   # (129: c = 8 stops with a margin of 5e-4 only)
TAIL129_CAP = 300
# the first B of these are the batches of the group-shape case: every edge length and 40...160, so that the
# groups hold sentences of 1 to 5 occupied slices side by side
GROUP_LENS = (97, 40, 1, 64, 2, 33, 160, 31, 65, 32, 120, 63, 96, 57, 48, 141,
              33, 129, 44, 100, 64, 81, 2, 152, 97, 72, 31, 110, 65, 135, 90, 128)
GROUP_BS = (1, 2, 3, 4, 5, 7, 8, 29, 32)
MEL_LENS = (40, 33, 2, 64, 40)
MEL_PAIRS = ((4, 4), (4, 5), (6, 6), (1, 1), (1, 5))   # nmel 320; queue 400; nmel 480; nmel 80; shift qo = 320


def _case(sents, cap=200, r=5, m=5, resident=True, oracle=None, crossing=None, reach=None, model_kw=None):
    sents = tuple(s if isinstance(s, Sent) else S(s) for s in sents)
    return dict(sents=sents, cap=cap, r=r, m=m, resident=resident, model_kw=dict(model_kw or {}),
                oracle=tuple(range(len(sents))) if oracle is None else tuple(oracle), crossing=dict(crossing or {}),
                reach=dict(reach or {}))


# name -> batch.  oracle: the sentences (indices) that go through the reference; crossing: index -> k, the slice
# boundary 32 k that at least half of the sentence's attention mass must move past within its steps; reach:
# index -> k, the slice the alignment argmax must arrive in (L = 65 and 97 have one position past their last
# boundary, where an unmodified sentence's alpha settles at 0.40 and 0.15: the argmax still gets there).
CASES = {
    # (a) one batch of three groups, the last with two sentences; every sentence also alone
    "slice_edges": _case(EDGE_LENS, crossing={4: 1, 5: 1, 6: 1, 7: 1, 8: 2, 9: 2}, reach={7: 2, 9: 3}),
    # (b) all seven boundaries
    "long": _case((255, 256), cap=500, crossing={0: 7, 1: 7}),
    # (c) the tail rule beyond slice 0, each tail sentence finishing while slot-mates go on
    "tail": _case((S(32, TAIL_FACTOR[32]), S(33, TAIL_FACTOR[33]), 40, S(64, TAIL_FACTOR[64]),
                   S(65, TAIL_FACTOR[65]), 97), crossing={1: 1, 3: 1, 4: 2}),
    "tail129": _case((S(129, TAIL_FACTOR[129]), 40, 97), cap=TAIL129_CAP, crossing={0: 4}),
    # (d) group shapes: slots 0, 1, 2, 3 of groups 0, 2, 4 and the last against the oracle
    "groups": _case(GROUP_LENS, cap=120, oracle=(0, 9, 18, 31)),
    # (f) where the resident path ends
    "b33": _case(GROUP_LENS + (33,), cap=120, resident=False, oracle=(9, 32)),
    "L257": _case((257, 40), resident=False),
    "queue560": _case((40, 33), cap=100, r=6, m=7, resident=False),
    "b32_L256": _case(GROUP_LENS[:31] + (256,), cap=120, oracle=(18, 31)),
    # (g) a handle smaller than the kernel's slices.  (The unmodified L = 17 sentence passes 0.6 with a tail of
    # 0.59955 one step earlier, inside MARGIN; with its last row x 16 it stops at step 32, 2.2e-2 clear.)
    "small_handle": _case((40, 33, 2, S(17, 16.0)), model_kw=dict(max_batch=4, max_len=40), crossing={0: 1}),
}
# (e) mel rows and queue: the B = 5 batch; sentence 0 also runs alone
for _r, _m in MEL_PAIRS:
    CASES[f"mel_r{_r}m{_m}"] = _case(MEL_LENS, cap=100, r=_r, m=_m, crossing={0: 1})


def flags(r, m, cap):
    fl = dict(golden_flags(golden("gst_L10_nostyle")))
    fl.update(r=r, memory_size=m, max_decoder_steps=cap)
    return fl


@functools.lru_cache(maxsize=None)
def _weights(r, m):
    return weights_mod().tacotron_gst_weights(0, r=r, memory_size=m)


@functools.lru_cache(maxsize=None)
def oracle(r, m, cap, f32=False, cls=None):
    from oracle.tacotron_oracle import TacotronOracle
    return (cls or TacotronOracle)(_weights(r, m), dtype=np.float32 if f32 else np.float64, **flags(r, m, cap))


@functools.lru_cache(maxsize=None)
def enc_rows(sent):
    """The sentence's encoder rows [L, 256] as float32 (read-only: shared by every test)."""
    e = oracle(5, 5, 200).encoder(weights_mod().synthetic_ids(sent.L, 900 + sent.L), None, None).astype(np.float32)
    e[-1] *= np.float32(sent.c)
    e.setflags(write=False)
    return e


def as_result(mel, stop, align):
    """An oracle decoder() return as the dict check_sentence compares."""
    return dict(mel=mel, stop=stop, align=align, steps=len(stop), frames=mel.shape[0])


@functools.lru_cache(maxsize=None)
def reference(sent, r=5, m=5, cap=200, f32=False):
    out = as_result(*oracle(r, m, cap, f32).decoder(enc_rows(sent)))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def case_reference(name, i, f32=False):
    c = CASES[name]
    return reference(c["sents"][i], c["r"], c["m"], c["cap"], f32)


def references():
    """Every (sentence, r, memory_size, cap) that a device test compares with the oracle, once, with the
    boundary its mass has to cross and the slice its argmax has to reach (0: none)."""
    seen = {}
    for name, c in CASES.items():
        for i in c["oracle"]:
            key = (c["sents"][i], c["r"], c["m"], c["cap"])
            have = seen.get(key, (0, 0))
            seen[key] = (max(have[0], c["crossing"].get(i, 0)), max(have[1], c["reach"].get(i, 0)))
    return seen


# ------------------------------------------------------------------ the comparison
def decisions(res, L):
    """The two halves of the stop rule per step as booleans (layers/tacotron.py:464-469): stop > 0.6, and
    alignment[-1] > 0.6 at the steps t > L / 4 (t counted from 1) where the rule is read."""
    stop = np.asarray(res["stop"], np.float64)[:res["steps"]]
    tail = np.asarray(res["align"], np.float64)[:res["steps"], L - 1]
    live = 4 * np.arange(1, res["steps"] + 1) > L
    return stop > 0.6, (tail > 0.6) & live


def tie_steps(ref_align):
    """Steps at which the oracle's own two largest alignment values are within TIE_GAP."""
    if ref_align.shape[1] < 2:
        return np.zeros(ref_align.shape[0], bool)
    top = np.partition(np.asarray(ref_align, np.float64), -2, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) <= TIE_GAP


def check_sentence(got, ref, L):
    """One sentence of a device (or faulted) run against the reference.  got / ref: dicts with steps, frames,
    mel [>= frames, 80], stop [>= steps], align [>= steps, >= L]; got may be padded as a batch pads it.
    Exact: step and frame count, every stop decision, the argmax of every step that is no near tie of the
    oracle's (at most SKIP_CAP of the steps may be one), zeros in alignment columns j >= L and in mel rows past
    the sentence's frames.  Alignment rows and stop values within ATOL max-abs, mel within RTOL relative RMS.
    (Stop and alignment rows past a sentence's steps are not part of a result: tests/test_gpu_tacotron_queue.py.)
    Returns the measured figures."""
    n, T = ref["steps"], ref["frames"]
    assert got["steps"] == n, f"step count {got['steps']} != {n}"
    assert got["frames"] == T, f"frame count {got['frames']} != {T}"
    align = np.asarray(got["align"])
    mel = np.asarray(got["mel"])
    stop = np.asarray(got["stop"])[:n]
    assert align.shape[0] >= n and align.shape[1] >= L and mel.shape[0] >= T and stop.shape[0] == n
    assert np.all(align[:n, L:] == 0), "alignment columns past the sentence's length must be zero"
    assert np.all(mel[T:] == 0), "mel rows past the sentence's frames must be zero"
    a, ra = align[:n, :L].astype(np.float64), np.asarray(ref["align"], np.float64)
    assert np.isfinite(a).all() and np.isfinite(stop).all() and np.isfinite(mel[:T]).all()
    for g, w, what in zip(decisions(got, L), decisions(ref, L), ("stop > 0.6", "alignment tail > 0.6")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    ties = tie_steps(ra)
    skipped = float(ties.mean())
    assert skipped <= SKIP_CAP, f"{skipped:.3f} of the steps are near ties of the oracle's argmax"
    np.testing.assert_array_equal(a.argmax(1)[~ties], ra.argmax(1)[~ties], err_msg="alignment argmax")
    fig = dict(align_err=float(np.abs(a - ra).max()),
               stop_err=float(np.abs(stop.astype(np.float64) - np.asarray(ref["stop"], np.float64)).max()),
               mel_rel_rms=rel_rms(mel[:T], ref["mel"]), skipped_argmax_share=skipped, steps=int(n))
    assert fig["align_err"] < ATOL, f"alignment max-abs {fig['align_err']:.3e}"
    assert fig["stop_err"] < ATOL, f"stop max-abs {fig['stop_err']:.3e}"
    assert fig["mel_rel_rms"] < RTOL, f"mel relative RMS {fig['mel_rel_rms']:.3e}"
    return fig


def worst(figs):
    """The largest of each figure over several sentences."""
    figs = list(figs)
    return {k: max(f[k] for f in figs) for k in ("align_err", "stop_err", "mel_rel_rms", "skipped_argmax_share")}


# ------------------------------------------------------------------ the device side
def make_model(r, m, cap, **kw):
    from conftest import load_pkg
    fl = flags(r, m, cap)
    mdl = load_pkg("tacotron").TacotronGST(
        130, fl["num_speakers"], r=r, memory_size=m, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
        forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"], forward_attn_mask=fl["forward_attn_mask"],
        location_attn=fl["location_attn"], prenet_type=fl.get("prenet_type", "original"), **kw)
    mdl.decoder.max_decoder_steps = cap
    return mdl.cuda().eval()


def batch_enc(sents, fill=0.0):
    """[B, Lmax, 256] float32 CPU tensor of the sentences' rows; rows j >= L hold `fill`."""
    import torch
    lens = [s.L for s in sents]
    enc = torch.full((len(sents), max(lens), 256), float(fill), dtype=torch.float32)
    for b, s in enumerate(sents):
        enc[b, :s.L] = torch.from_numpy(np.array(enc_rows(s)))
    return enc, lens


def run(model, sents, cap, fill=0.0):
    """Decode the batch on the device; numpy results plus the serving path."""
    model.decoder.max_decoder_steps = cap
    enc, lens = batch_enc(sents, fill)
    out = model.inference_batch(None, enc=enc.cuda(), lens=lens, postnet=False)
    return dict(mel=out["mel"].cpu().numpy(), align=out["align"].cpu().numpy(), stop=out["stop"].cpu().numpy(),
                steps=list(out["steps"]), frames=list(out["frames"]), lens=lens,
                resident=model.last_timing["resident"])


def run_case(model, name, fill=0.0, first=None):
    c = CASES[name]
    return run(model, c["sents"][:first], c["cap"], fill)


def sentence(res, b):
    """Sentence b of a run() result as check_sentence takes it (padded as the batch pads it)."""
    return dict(mel=res["mel"][b], align=res["align"][b], stop=res["stop"][b, :res["steps"][b]],
                steps=res["steps"][b], frames=res["frames"][b])


def trimmed(x, L):
    """A sentence() result cut to its own steps, frames and length: a reference for check_sentence."""
    n, T = x["steps"], x["frames"]
    return dict(mel=x["mel"][:T], align=x["align"][:n, :L], stop=x["stop"][:n], steps=n, frames=T)


def same_bits(x, y, L):
    """Sentence results x, y (sentence()) carry the same bits: counts, mel, stop and alignment over the steps."""
    n, T = x["steps"], x["frames"]
    return (n == y["steps"] and T == y["frames"] and np.array_equal(x["mel"][:T], y["mel"][:T])
            and np.array_equal(x["stop"][:n], y["stop"][:n])
            and np.array_equal(x["align"][:n, :L], y["align"][:n, :L]))
