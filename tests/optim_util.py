"""Shared by tests/golden/make_golden_optim.py, test_optim_cpu.py and test_gpu_optim.py: the tensor set and the
seeded inputs of the optim.npz fixture (regenerated from seeds, never stored), a numpy float32 restatement of
csrc/optim.hip's exact operation order, an fp64 evaluation of the same formulas, and the error bounds.

The restatement (``step_f32``), per element, one float32 rounding per operation, in this order:
  1. p = p + dlr * p                     dlr = float32(-wd * lr); skipped when wd == 0; every tensor
  2. g = g * coef                        only when coef != 1; coef = float32(max_norm / (norm + 1e-6)) where that
                                         fp64 quotient is below 1, else 1
  3. m = m + w1 * (g - m)                w1 = float32(1 - beta1) (< 0.5: ATen's lerp form for such a weight)
     v = v * beta2; v = v + (w2 * g) * g w2 = float32(1 - beta2)
     d = sqrt(v) / sqrt(bc2) + eps
     p = p + (nstep * m) / d             nstep = float32(-(lr / bc1)), bc = 1 - beta ** step in double
A tensor without a gradient takes part in 1 only and its step does not advance.

Bounds, in units of u = 2^-24, the units from the error model (one rounding per float32 operation):
  m' within k_m u (|m| + |g|)            lerp: the subtraction, the product and the sum round once each, each
                                         below u (|m| + |g|); the cancellation in g - m is bounded by its operands
  v' within k_v u v'                     three roundings of non-negative terms that only add
  p' within u |p'| + k_p u |dp|          the last sum's rounding, plus the Adam update dp (fp64 evaluation) with
                                         its roundings: the scalar constants, m', the root, two divisions, the
                                         sum with eps, the product.  (A decay that moves p, |dlr| >= 2^-25, case
                                         (e) only, rounds once more at the magnitude of p: 2 u |p'| there.)
The constants are measured, not modelled, on the fixture (real torch CPU, foreach=False), every case and
iteration, each iteration from torch's own previous state (test_optim_cpu.py prints the figures):

  K, the distance restatement <-> torch: MEASURED_GAP is the largest observed, K twice that, because torch's
  vectorised CPU kernels fuse a multiply-add where the restatement does not (iteration 0, m = v = 0, is
  bitwise equal; later ones are not).  k_v is dominated by the clipping cases: torch forms its coefficient
  from its float32 norm, up to 8 u from the fp64 one.  k_p is dominated by elements whose float32 p' falls on
  the other side of a rounding boundary, a whole ulp of p' for a change of dp by u |dp|: that is a property
  of comparing two float32 results directly, not of either.

  K64, the distance of ONE float32 result from the fp64 evaluation of the same inputs (with the clip
  coefficient that result used): MEASURED_TORCH is the largest observed for torch's values, K64 twice that.
  The restatement's own figures (m 0.849, v 3.720, p 2.938) lie inside.  This is the bound for comparing with
  a torch that computes in another order (the GPU kernels): both results within K64 of the fp64 evaluation.
  All constants were measured on the fixture's sampled elements (about 800 per iteration).  p's unit u |dp|
  does not hold over a much larger population: dp is proportional to m', whose error is bounded by |m| + |g|
  and not by |m'|, so where m' cancels the ratio grows (about 100 over 110 970 elements, for torch as for the
  device).  m's and v's units hold at every element.
"""
import math

import numpy as np

CHUNK = 8192
F = np.float32
U = 2.0 ** -24

# index -> elements; NONE has no gradient, VIEW is taken at element offset 1 of a larger buffer
SIZES = (1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 70001, 257, 5003)
NONE, VIEW = 7, 8
BETAS, EPS = (0.9, 0.999), 1e-8
WARMUP = 4000
SCHEDULE_STEPS = (0, 1, WARMUP - 1, WARMUP, WARMUP + 1, 10 * WARMUP)
ITERATIONS = 3

# case -> lr, wd, grad_clip, gradient scale, restored step (0: fresh state), NoamLR driven
CASES = {
    "a": dict(lr=1e-3, wd=1e-6, grad_clip=1e3, gscale=1e-2, step0=0, noam=False),    # no clipping
    "b": dict(lr=1e-3, wd=1e-6, grad_clip=1.0, gscale=1e-2, step0=0, noam=False),    # norm ~ 3.3: clipping
    "c": dict(lr=1e-3, wd=1e-6, grad_clip=1.0, gscale=1e-12, step0=0, noam=False),   # eps dominates
    "d": dict(lr=1e-3, wd=1e-6, grad_clip=1.0, gscale=1e-2, step0=1000, noam=True),  # restored state, NoamLR
    "e": dict(lr=1e-3, wd=5e-2, grad_clip=1e3, gscale=1e-2, step0=0, noam=False),    # a decay that moves p
}
SEEDS = {c: 1000 * (i + 1) for i, c in enumerate(CASES)}

MEASURED_GAP = dict(m=1.589, v=16.800, p=149.420)
K = dict(m=3.2, v=33.6, p=299.0)
MEASURED_TORCH = dict(m=0.775, v=3.371, p=2.938)
K64 = dict(m=1.55, v=6.75, p=5.9)


def initial_state(case):
    """(p, m, v, steps): lists over SIZES of float32 arrays, and the step each tensor has taken."""
    cfg = CASES[case]
    g = np.random.Generator(np.random.PCG64(SEEDS[case]))
    p = [(0.1 * g.standard_normal(n)).astype(F) for n in SIZES]
    if cfg["step0"]:
        m = [(0.3 * cfg["gscale"] * g.standard_normal(n)).astype(F) for n in SIZES]
        v = [(cfg["gscale"] ** 2 * g.uniform(0.2, 1.0, n)).astype(F) for n in SIZES]
    else:
        m = [np.zeros(n, F) for n in SIZES]
        v = [np.zeros(n, F) for n in SIZES]
    return p, m, v, [cfg["step0"]] * len(SIZES)


def gradients(case, it):
    """The gradients of iteration ``it`` (0-based): a list over SIZES, None for the tensor without one."""
    g = np.random.Generator(np.random.PCG64(SEEDS[case] + 1 + it))
    out = [(CASES[case]["gscale"] * g.standard_normal(n)).astype(F) for n in SIZES]
    out[NONE] = None
    return out


def sample_indices(n):
    """The elements of an n-element tensor whose torch results the fixture stores: all of a small tensor; else
    both ends, both sides of every chunk boundary, and 96 more by seed."""
    if n <= 16:
        return np.arange(n)
    idx = {0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1}
    for b in range(CHUNK, n, CHUNK):
        idx.update((b - 2, b - 1, b, b + 1))
    idx.update(np.random.Generator(np.random.PCG64(n)).integers(0, n, 96).tolist())
    return np.array(sorted(i for i in idx if 0 <= i < n))


def noam_lr(base_lr, last_epoch, warmup=WARMUP):
    step = max(last_epoch, 1)
    return base_lr * float(warmup) ** 0.5 * min(step * float(warmup) ** -1.5, step ** -0.5)


# ------------------------------------------------------------------ the norm
def norm64(grads):
    """sqrt of the correctly rounded (math.fsum) sum of g * g in float64, over the tensors that have a gradient;
    and the number of terms."""
    sq = [np.square(g.astype(np.float64)) for g in grads if g is not None]  # (each square is exact in float64)
    n = int(sum(s.size for s in sq))
    return math.sqrt(math.fsum(math.fsum(s.tolist()) for s in sq)), n


def norm_bound(n_terms):
    return (n_terms + 4) * 2.0 ** -52


def clip_coef(norm, max_norm):
    with np.errstate(all="ignore"):
        q = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return F(1.0) if q >= 1.0 else F(q)  # (a NaN quotient stays NaN, as torch's clamp keeps it)


def adam_scalars(lr, step, betas=BETAS, eps=EPS):
    """The per-tensor scalars of update number ``step`` (>= 1): doubles as torch/optim/adam.py forms them."""
    bc1, bc2 = 1 - betas[0] ** float(step), 1 - betas[1] ** float(step)
    return dict(w1=1 - betas[0], beta2=betas[1], w2=1 - betas[1], sqrt_bc2=bc2 ** 0.5, nstep=-(lr / bc1), eps=eps)


# ------------------------------------------------------------------ one iteration, float32 as the device does it
def element_f32(p, g, m, v, dlr, coef, sc):
    """One tensor: (p', g', m', v') from float32 arrays; dlr None skips the decay, g None all but the decay."""
    with np.errstate(all="ignore"):
        if dlr is not None:
            p = p + F(dlr) * p
        if g is None:
            return p, None, m, v
        if coef != F(1.0):
            g = g * coef
        w1 = F(sc["w1"])
        d = g - m
        m = m + w1 * d if w1 < F(0.5) else g - d * (F(1.0) - w1)
        v = v * F(sc["beta2"])
        v = v + (F(sc["w2"]) * g) * g
        denom = np.sqrt(v) / F(sc["sqrt_bc2"]) + F(sc["eps"])
        p = p + (F(sc["nstep"]) * m) / denom
    for a in (p, g, m, v):
        assert a.dtype == F
    return p, g, m, v


def step_f32(p, g, m, v, steps, lr, wd, grad_clip, norm=None):
    """weight_decay, check_update, optimizer.step on lists of float32 arrays.  Returns (p, g, m, v, steps, norm):
    new lists, the inputs are left alone.  ``norm`` defaults to norm64 of the gradients."""
    if norm is None:
        norm = norm64(g)[0]
    coef = clip_coef(norm, grad_clip)
    dlr = -wd * lr if wd != 0 else None
    out = ([], [], [], [], [])
    for pi, gi, mi, vi, si in zip(p, g, m, v, steps):
        s2 = si + (gi is not None)
        r = element_f32(pi, gi, mi, vi, dlr, coef, adam_scalars(lr, s2) if gi is not None else None)
        for o, x in zip(out, r + (s2,)):
            o.append(x)
    return out + (norm,)


# ------------------------------------------------------------------ the same formulas in float64
def element_f64(p, g, m, v, lr, wd, coef, step):
    """float64 evaluation from the float32 inputs (coef: the float32 coefficient): (p', g', m', v', dp), dp the
    Adam update alone."""
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    b1, b2 = BETAS
    p1 = p + (-wd * lr) * p
    g = g * float(coef)
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    dp = -(lr / (1 - b1 ** step)) * m2 / (np.sqrt(v2) / math.sqrt(1 - b2 ** step) + EPS)
    return p1 + dp, g, m2, v2, dp


def torch_clip_coef(norm32, max_norm):
    """clip_grad_norm_'s own coefficient from the float32 norm it returned: float32 arithmetic throughout."""
    q = F(max_norm) / (F(norm32) + F(1e-6))
    return F(1.0) if q >= 1.0 else q


def ratios(got, ref, p, g, m, v, lr, wd, coef, step):
    """The largest distance of ``got`` = (p', m', v') from ``ref`` = (p', m', v') in the units of the docstring:
    dict(m=, v=, p=).  p, g, m, v are the float32 inputs of the iteration; the units come from their fp64
    evaluation with the coefficient ``coef``.  A decay that moves p (|dlr| >= 2^-25) rounds once more at the
    magnitude of p, so the first term of p's bound counts twice then."""
    p64, g64, m64, v64, dp = element_f64(p, g, m, v, lr, wd, coef, step)
    gp, gm, gv = (np.asarray(x, np.float64) for x in got)
    rp, rm, rv = (np.asarray(x, np.float64) for x in ref)
    tiny = 1e-300
    rounds = 2.0 if abs(wd * lr) >= 2.0 ** -25 else 1.0
    km = np.max(np.abs(gm - rm) / (U * (np.abs(m.astype(np.float64)) + np.abs(g64)) + tiny))
    kv = np.max(np.abs(gv - rv) / (U * np.abs(v64) + tiny))
    kp = np.max(np.maximum(np.abs(gp - rp) - rounds * U * np.abs(p64), 0.0) / (U * np.abs(dp) + tiny))
    return dict(m=float(km), v=float(kv), p=float(kp))
