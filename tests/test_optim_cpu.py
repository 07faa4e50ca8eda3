"""CPU: the numpy restatement of csrc/optim.hip's arithmetic (optim_util.py) against real torch (optim.npz:
the reference's weight_decay / check_update and torch.optim.Adam on CPU, tests/golden/make_golden_optim.py),
the norm rule, the schedules, and optim.Adam's argument checks.  Nothing here needs a device.

Every iteration is checked on its own: iteration k starts from TORCH's state after iteration k - 1 (the
fixture's), never from a trajectory of the restatement.  Bounds and their constants: optim_util.py.
"""
import math
import warnings

import numpy as np
import pytest
import torch

import optim_util as ou
from conftest import REPO, golden, load_pkg

Z = golden("optim")
F = np.float32


def torch_state(case, it):
    """Torch's (p, m, v) at the sampled elements before iteration ``it``, lists over SIZES (m, v None where
    torch holds no state)."""
    if it == 0:
        p, m, v, _ = ou.initial_state(case)
        idx = [ou.sample_indices(n) for n in ou.SIZES]
        return [a[i] for a, i in zip(p, idx)], [a[i] for a, i in zip(m, idx)], [a[i] for a, i in zip(v, idx)]
    key = f"{case}{it - 1}"
    n = len(ou.SIZES)
    return ([Z[f"{key}_p{i}"] for i in range(n)], [Z[f"{key}_m{i}"] if f"{key}_m{i}" in Z else None for i in range(n)],
            [Z[f"{key}_v{i}"] if f"{key}_v{i}" in Z else None for i in range(n)])


def one_iteration(case, it):
    """The restatement's and torch's results of iteration ``it`` at the sampled elements, and the inputs:
    yields (i, got (p, g, m, v), ref (p, g, m, v), inputs (p, g, m, v), lr, coef, step) per tensor."""
    cfg = ou.CASES[case]
    key = f"{case}{it}"
    lr = float(Z[key + "_lr"])
    grads = ou.gradients(case, it)
    norm, _ = ou.norm64(grads)
    coef = ou.clip_coef(norm, cfg["grad_clip"])
    p, m, v = torch_state(case, it)
    for i, n in enumerate(ou.SIZES):
        idx = ou.sample_indices(n)
        step = int(Z[key + "_steps"][i])
        if grads[i] is None:
            got = ou.element_f32(p[i], None, m[i], v[i], -cfg["wd"] * lr, coef, None)
            yield i, got, (Z[f"{key}_p{i}"], None, Z.get(f"{key}_m{i}"), Z.get(f"{key}_v{i}")), None, lr, coef, step
            continue
        g = grads[i][idx]
        got = ou.element_f32(p[i], g, m[i], v[i], -cfg["wd"] * lr, coef, ou.adam_scalars(lr, step))
        ref = tuple(Z[f"{key}_{a}{i}"] for a in "pgmv")
        yield i, got, ref, (p[i], g, m[i], v[i]), lr, coef, step


@pytest.mark.parametrize("it", range(ou.ITERATIONS))
@pytest.mark.parametrize("case", list(ou.CASES))
def test_restatement_against_torch(case, it):
    cfg = ou.CASES[case]
    ref32 = float(Z[f"{case}{it}_norm"])
    ref64 = ou.norm64(ou.gradients(case, it))[0]
    tcoef = ou.torch_clip_coef(ref32, cfg["grad_clip"])
    gap, own, tor = (dict(m=0.0, v=0.0, p=0.0) for _ in range(3))
    for i, got, ref, inputs, lr, coef, step in one_iteration(case, it):
        if inputs is None:  # no gradient: the decay alone, state and step as they were
            assert np.array_equal(got[0], ref[0]) and step == cfg["step0"]
            if ref[2] is not None:
                assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
            continue
        assert step == cfg["step0"] + it + 1
        if coef == F(1.0):
            assert tcoef == F(1.0) and np.array_equal(got[1], inputs[1]) and np.array_equal(ref[1], inputs[1])
        # the clipped gradient: torch forms its coefficient in float32 from ITS float32 norm, the device in float64
        # from the fp64 norm, rounded once: the norms' distance, the roundings of the sum with 1e-6, of the
        # quotient and of its conversion, and one product rounding on each side
        rel = abs(ref32 - ref64) / ref64 + 5 * ou.U
        assert np.all(np.abs(got[1].astype(np.float64) - ref[1]) <= rel * np.abs(ref[1]))
        args = (lr, cfg["wd"], coef, step)
        for acc, a, b, c in ((gap, got, ref, coef), (own, got, None, coef), (tor, ref, None, tcoef)):
            if b is None:
                e = ou.element_f64(*inputs, lr, cfg["wd"], c, step)
                b = (e[0], None, e[2], e[3])
            r = ou.ratios((a[0], a[2], a[3]), (b[0], b[2], b[3]), *inputs, lr, cfg["wd"], c, step)
            for k in acc:
                acc[k] = max(acc[k], r[k])
    fmt = lambda d: ", ".join(f"k_{k} {x:.3f}" for k, x in d.items())
    print(f"{case}{it} (units of 2^-24): restatement against torch {fmt(gap)}; against its fp64 evaluation {fmt(own)}; "
          f"torch against its fp64 evaluation {fmt(tor)}")
    for k in gap:
        assert gap[k] <= ou.K[k], (k, gap[k])
        assert own[k] <= ou.K64[k] and tor[k] <= ou.K64[k], (k, own[k], tor[k])


def test_decay_moves_the_parameters_in_case_e_only():
    """wd = 1e-6 at lr = 1e-3 is below half an ulp of p (the reference's own config, a bit-neutral decay);
    case (e) is there so that the decay is seen at all."""
    for case in ou.CASES:
        p = ou.initial_state(case)[0][ou.NONE]
        q = ou.element_f32(p, None, None, None, -ou.CASES[case]["wd"] * ou.CASES[case]["lr"], F(1.0), None)[0]
        assert np.array_equal(p, q) == (case != "e")


@pytest.mark.parametrize("case", list(ou.CASES))
def test_norm(case):
    for it in range(ou.ITERATIONS):
        grads = ou.gradients(case, it)
        ref64, n = ou.norm64(grads)
        assert n == sum(s for i, s in enumerate(ou.SIZES) if i != ou.NONE)
        value = math.sqrt(sum(float(np.dot(g.astype(np.float64), g.astype(np.float64))) for g in grads if g is not None))
        assert abs(value - ref64) <= ou.norm_bound(n) * ref64  # a float64 sum in another order
        ref32 = float(Z[f"{case}{it}_norm"])
        print(f"{case}{it}: fp64 norm {ref64!r}, torch's float32 {ref32!r}")
        # torch's float32 norm: a float32 sum of N non-negative terms in any order is within (N + 2) u of the sum
        assert abs(ref32 - ref64) <= (n + 2) * ou.U * ref64
        # eval_util.py's rule for the float32 scalar: the fp64 value rounded once against torch's float32 one
        assert abs(float(F(ref64)) - ref32) <= abs(ref32 - ref64) + 2.0 ** -23 * ref64


def test_schedules_equal_the_reference():
    gu = load_pkg("generic_utils")
    optim = load_pkg("optim")
    assert [gu.lr_decay(1e-3, s, ou.WARMUP) for s in ou.SCHEDULE_STEPS] == Z["lr_decay"].tolist()
    opt = optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)  # (no device is needed to build one)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scheduler.step() before optimizer.step(), as train.py:119-120 has it
        sch = gu.NoamLR(opt, warmup_steps=ou.WARMUP, last_epoch=-1)
        vals = {0: opt.param_groups[0]["lr"]}
        for s in range(1, max(ou.SCHEDULE_STEPS) + 1):
            sch.step()
            if s in ou.SCHEDULE_STEPS:
                vals[s] = opt.param_groups[0]["lr"]
    assert [vals[s] for s in ou.SCHEDULE_STEPS] == Z["noam_lr"].tolist()
    assert ou.noam_lr(1e-3, 1001) == float(Z["d0_lr"])  # case (d): restored at 1000, stepped before the iteration
    assert gu.mk_decay(2.0, 10, 3) == 2.0 * ((10 - 3) / 10)
    lin = torch.nn.Linear(3, 4)
    lin.bias.requires_grad_(False)
    assert gu.count_parameters(lin) == 12


def test_adam_argument_checks():
    optim = load_pkg("optim")
    P = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError):
        optim.Adam(P, amsgrad=True)
    for bad in (dict(weight_decay=1e-2), dict(lr=0.0), dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                dict(eps=-1e-8)):
        with pytest.raises(ValueError):
            optim.Adam(P, **bad)
    with pytest.raises(ValueError, match="one param group"):
        optim.Adam([dict(params=P), dict(params=[torch.nn.Parameter(torch.zeros(2))])])
    with pytest.raises(ValueError, match="float32"):
        optim.Adam([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, 4).t()[1:])])
    opt = optim.Adam(P, lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (2e-3, (0.8, 0.99), 1e-7, 0, False)
    assert opt.state_dict()["state"] == {} and opt.last_norm is None
    torch.optim.Adam(P).load_state_dict(opt.state_dict())  # torch.optim.Adam's own group keys
    opt.load_state_dict(torch.optim.Adam(P).state_dict())
    assert optim.CHUNK == ou.CHUNK == int(__import__("re").search(r"#define TTS_OPTIM_CHUNK (\d+)", open(
        REPO + "/include/tts_hip.h").read()).group(1))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    optim, gu = load_pkg("optim"), load_pkg("generic_utils")
    P = [torch.nn.Parameter(torch.zeros(3))]
    P[0].grad = torch.ones(3)
    opt = optim.Adam(P)
    for call in (opt.step, lambda: opt.step_fused(1e-6, 1.0), lambda: gu.weight_decay(opt, 1e-6),
                 lambda: gu.check_update(P, 1.0)):
        with pytest.raises(RuntimeError, match="no GPU"):
            call()
    assert not opt.state[P[0]] or int(opt.state[P[0]]["step"]) == 0
