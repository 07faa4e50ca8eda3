"""Shared by tests/golden/make_golden_loss_grad.py, test_loss_grad_cpu.py and test_gpu_loss_grad.py: the inputs
of the loss_grad.npz fixture (regenerated from seeds, never stored), the index sample the large cases are
stored at, a float64 numpy restatement of the three gradients, and the two bounds of the GPU test.

Bounds.  The device forms a gradient in fp64 and rounds it to fp32 once, so against the restatement g64

    |got - g64| <= 2^-24 |g64| (1 + 2^-20)

half an fp32 ulp of that rounding, with slack for the order of the (two or three) fp64 operations.  Against the
reference's float32 gradient, which carries its own float32 roundings, the reference's own error is the
allowance: |got - ref32| <= |ref32 - ref64| + 2^-24 |ref64| (1 + 2^-20).  BCE adds an absolute
4 * 2^-53 * |k| / n to both: ``sigmoid(x) - y`` cancels at x = +-100, where an ulp of the sigmoid is all that is
left (and a product below the smallest float32 rounds to 0).
"""
import numpy as np

import eval_util as eu

CHUNK = 8192  # LOSS_CHUNK of csrc/losses.hip
UPSTREAM = (1.0, 0.375)  # the second through (0.375 * loss).backward()
KINDS = ("l1", "mse")

# name -> (seed, (B, T, D), lengths); the cases of eval_util.py come first
CASES = dict(eu.LOSS_CASES)
CASES["g"] = (106, (3, 9, 1025), [9, 0, 8])  # 9225 elements: over the chunk edge, a partial last quad; an empty sentence
CASES["h"] = (107, (2, 5, 3), [5, 2])        # T * D = 15, no multiple of four
SAMPLED = ("b", "g")  # stored at sample_indices(), the others in full
TIE_SEED = 108
RUNS = [(case, kind, name) for case, (_, _, lengths) in CASES.items() for kind in KINDS
        for name in (("plain", "masked") if lengths is not None else ("plain",))]


def inputs(case):
    """(x, y, lengths) of a case.  In ``g`` a seeded 1 % of the valid elements have x == y (the L1 tie)."""
    if case in eu.LOSS_CASES:
        return eu.loss_inputs(case)
    seed, shape, lengths = CASES[case]
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal(shape).astype(np.float32)
    y = g.uniform(-1.0, 1.0, shape).astype(np.float32)
    if case == "g":
        tie = ties(case)
        x[tie] = y[tie]
    return x, y, lengths


def valid_mask(shape, lengths):
    B, T, D = shape
    rows = np.full(B, T) if lengths is None else np.minimum(np.asarray(lengths), T)
    return np.broadcast_to((np.arange(T)[None, :] < rows[:, None])[:, :, None], shape)


def ties(case):
    _, shape, lengths = CASES[case]
    draw = np.random.Generator(np.random.PCG64(TIE_SEED)).random(shape) < 0.01
    return draw & valid_mask(shape, lengths)


def sample_indices(case):
    """Flat indices into [B * T * D] a sampled case is stored at: every chunk edge of every sentence +- 4 elements,
    every n[b] +- 4, the sentence's two ends, and 2000 seeded indices."""
    seed, (B, T, D), lengths = CASES[case]
    per = T * D
    idx = set(int(v) for v in np.random.Generator(np.random.PCG64(seed + 1000)).integers(0, B * per, 2000))
    for b in range(B):
        marks = list(range(0, per + 1, CHUNK)) + [min(lengths[b], T) * D, per]
        for m in marks:
            idx.update(b * per + e for e in range(m - 4, m + 4) if 0 <= e < per)
    return np.array(sorted(idx), dtype=np.int64)


def stored(case, grad):
    """What the fixture holds of a [B, T, D] gradient."""
    flat = np.asarray(grad).reshape(-1)
    return flat[sample_indices(case)] if case in SAMPLED else flat


def key(case, kind, name, k):
    return f"{case}_{kind}_{name}_k{UPSTREAM.index(k)}"


# ------------------------------------------------------------------ the gradients, restated in float64
def elementwise_grad(kind, x, y, lengths, k):
    """d (k * loss) / d x of L1LossMasked / MSELossMasked (lengths given) or nn.L1Loss / nn.MSELoss (None) on
    [B, T, D], float64 from the float32 operands: k * sign(x - y) / count or k * 2 (x - y) / count on the valid
    elements, 0 on the padding; NaN everywhere when count is 0 (the reference's inf * 0)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mask = valid_mask(x.shape, lengths)
    count = int(mask.sum())
    if count == 0:
        return np.full(x.shape, np.nan)
    d = x - y
    scale = np.float64(k) / np.float64(count)
    return np.where(mask, scale * (np.sign(d) if kind == "l1" else 2.0 * d), 0.0)


def bce_grad(x, y, k):
    """d (k * BCEWithLogitsLoss) / d x: k * (sigmoid(x) - y) / n, the sigmoid without overflow."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    e = np.exp(-np.abs(x))
    sg = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return (np.float64(k) / np.float64(x.size)) * (sg - y)


# ------------------------------------------------------------------ the bounds
F64_AGREE = 4 * 2.0 ** -53  # the restatement against the reference's float64 gradient, relative


def bce_abs(k, n):
    return 4 * 2.0 ** -53 * abs(k) / n


def restated_bound(g64, absolute=0.0):
    return 2.0 ** -24 * np.abs(g64) * (1 + 2.0 ** -20) + absolute


def reference_bound(ref32, ref64, absolute=0.0):
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    return np.abs(ref32 - ref64) + restated_bound(ref64, absolute)


def check_gradient(got, g64, ref32=None, ref64=None, absolute=0.0, what=""):
    """``got`` (float32, any shape) against the restatement ``g64`` of the same shape, and, where given, against the
    reference's two gradients (all three at the same elements).  Prints the figures before it asserts."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(g64), (got.dtype, got.shape)
    if np.isnan(g64).any():
        assert np.isnan(g64).all() and np.isnan(got).all(), what
        assert ref64 is None or (np.isnan(ref32).all() and np.isnan(ref64).all()), what
        print(f"{what}: all NaN")
        return
    err = np.abs(got.astype(np.float64) - g64)
    bound = restated_bound(g64, absolute)
    line = f"{what}: worst |got - g64| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}"
    if ref64 is not None:
        err_r = np.abs(got.astype(np.float64) - np.asarray(ref32, np.float64))
        bound_r = reference_bound(ref32, ref64, absolute)
        line += f", worst |got - ref32| / bound {float((err_r / np.maximum(bound_r, 1e-300)).max()):.3f}"
    print(line)
    assert (err <= bound).all(), what
    if ref64 is not None:
        assert (err_r <= bound_r).all(), what
