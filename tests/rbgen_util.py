"""Helpers of the rbgen_* fixture tests (tests/golden/make_golden_resident_batch_general.py): the
pool files of the resident batch decoder's general attention form and the argmax rule.

The argmax rule: under softmax the untrained weights give near-uniform alignments with near-ties.  A
max-abs error below ALIGN_ATOL = 4e-6 cannot swap two entries whose reference gap is >= 8e-6, so the
per-step argmax is asserted at the steps whose reference top-2 gap is >= ARGMAX_GAP = 2 x ALIGN_ATOL
only; the steps left out are capped per sentence at the larger of 2 steps and 1 % of the steps.
"""
import numpy as np

from conftest import golden, golden_flags

ALIGN_ATOL = 4e-6
ARGMAX_GAP = 2 * ALIGN_ATOL
CONFIGS = ("loc_softmax", "loc_fwd_ta", "loc_fwd_ta_mask", "win_fwdmask", "win_softmax")
LENGTHS = {c: (2, 20, 33, 129, 256) if c in ("loc_softmax", "loc_fwd_ta") else (2, 20, 33, 129) for c in CONFIGS}
KEYS = ("ids", "enc", "mel", "mel_post", "align", "stop")


def rbgen_file(config, L):
    """The pool file of sentence L (the L = 256 sentences have files of their own: size)."""
    return f"rbgen_{config}_L256" if L == 256 else f"rbgen_{config}"


def rbgen(config, L):
    """Sentence L of a configuration's pool: ids, enc and the reference's outputs."""
    z = golden(rbgen_file(config, L))
    return {k: z[f"{k}_L{L}"] for k in KEYS}


def rbgen_flags(config):
    return golden_flags(golden(f"rbgen_{config}"))


def decided_steps(ref_align):
    """Boolean [T]: the steps whose reference top-2 gap is >= ARGMAX_GAP (the argmax is asserted there)."""
    top = np.sort(np.asarray(ref_align, np.float64), axis=1)
    return top[:, -1] - top[:, -2] >= ARGMAX_GAP


def left_out_cap(steps):
    return max(2, steps // 100)


def assert_argmax(align, ref_align, what=""):
    """The argmax rule, with the cap on the left-out steps rechecked on the reference."""
    keep = decided_steps(ref_align)
    assert (~keep).sum() <= left_out_cap(len(keep)), f"{what}: {(~keep).sum()} steps left out"
    np.testing.assert_array_equal(np.asarray(align).argmax(1)[keep], np.asarray(ref_align).argmax(1)[keep], err_msg=what)
