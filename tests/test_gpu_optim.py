"""The training update on the device (csrc/optim.hip through optim.Adam and generic_utils.weight_decay /
check_update) against the numpy float32 restatement of its exact operation order (optim_util.py, bitwise) and
against real torch (optim.npz: the reference's helpers and torch.optim.Adam on CPU, make_golden_optim.py).

Bounds: optim_util.py.  K is the distance to the fixture's torch values (same constants as test_optim_cpu.py);
K64 the distance of one float32 result from the fp64 evaluation of its inputs, used where the other side is
torch's GPU Adam, which computes in another order than torch's CPU one.  The norm: the fp64 value within
(N + 4) * 2^-52 relative of the math.fsum value of the same gradients, the float32 one its rounding.
"""
import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import optim_util as ou
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu
Z = golden("optim")
F = np.float32
N_GRAD = sum(n for i, n in enumerate(ou.SIZES) if i != ou.NONE)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_params(arrays, views=(ou.VIEW,)):
    """Parameters over the arrays; those in ``views`` at element offset 1 of a larger buffer (4-byte aligned)."""
    out = []
    for i, a in enumerate(arrays):
        if i in views:
            buf = torch.zeros(a.size + 8, device="cuda")
            buf[1:1 + a.size] = dev(a)
            t = buf[1:1 + a.size]
            assert t.data_ptr() % 16 == 4
        else:
            t = dev(a)
            assert t.data_ptr() % 16 == 0
        out.append(torch.nn.Parameter(t))
    return out


def make_adam(p, m, v, steps, lr, views=(ou.VIEW,)):
    """optim.Adam over device copies of p, with the state (m, v, steps) restored where a step has been taken."""
    params = make_params(p, views)
    opt = load_pkg("optim").Adam(params, lr=lr, betas=ou.BETAS, eps=ou.EPS)
    for P, mi, vi, s in zip(params, m, v, steps):
        if s:
            opt.state[P] = dict(step=torch.tensor(float(s)), exp_avg=dev(mi), exp_avg_sq=dev(vi))
    return opt, params


def set_grads(params, grads):
    """A new allocation for every gradient; the old ones are kept alive so that no address comes back."""
    old = [P.grad for P in params]
    for P, g in zip(params, grads):
        P.grad = None if g is None else dev(g)
    set_grads.keep = getattr(set_grads, "keep", []) + old
    for P, o in zip(params, old):
        assert o is None or P.grad is None or o.data_ptr() != P.grad.data_ptr()


def read(opt, params):
    """(p, g, m, v, steps) as numpy lists; m, v None and step 0 where the optimizer holds no state."""
    torch.cuda.synchronize()
    st = [opt.state.get(P, {}) for P in params]
    return ([P.detach().cpu().numpy() for P in params], [None if P.grad is None else P.grad.cpu().numpy() for P in params],
            [s["exp_avg"].cpu().numpy() if s else None for s in st],
            [s["exp_avg_sq"].cpu().numpy() if s else None for s in st], [int(s["step"]) if s else 0 for s in st])


def same(got, want, what=""):
    """Bitwise equality of two lists of arrays (None matches None or an all-zero state never made)."""
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and (b is None or not np.any(b)), (what, i)
        else:
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, i)


def check_norm(opt, grad_norm, grads, n_terms):
    ref64 = ou.norm64(grads)[0]
    got64, got32 = float(opt.last_norm64), grad_norm.cpu().numpy()
    assert grad_norm.shape == () and grad_norm.dtype == torch.float32 and grad_norm.is_cuda
    print(f"norm {got64!r} ref {ref64!r} rel err {abs(got64 - ref64) / ref64:.3e} bound {ou.norm_bound(n_terms):.3e}")
    assert abs(got64 - ref64) <= ou.norm_bound(n_terms) * ref64
    assert got32 == F(got64)
    return got64


@functools.lru_cache(maxsize=None)
def run_case(case):
    """Three fused iterations of a fixture case from its initial state, and the restatement's trajectory:
    a list of (device (p, g, m, v, steps), restatement (p, g, m, v, steps), inputs g)."""
    gu = load_pkg("generic_utils")
    cfg = ou.CASES[case]
    p, m, v, steps = ou.initial_state(case)
    opt, params = make_adam(p, m, v, steps, cfg["lr"])
    sch = None
    if cfg["noam"]:
        opt.param_groups[0]["initial_lr"] = cfg["lr"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sch = gu.NoamLR(opt, warmup_steps=ou.WARMUP, last_epoch=cfg["step0"] - 1)
    out = []
    for it in range(ou.ITERATIONS):
        if sch is not None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sch.step()
        g = ou.gradients(case, it)
        set_grads(params, g)
        grad_norm, lr = opt.step_fused(cfg["wd"], cfg["grad_clip"])
        assert lr == float(Z[f"{case}{it}_lr"])  # NoamLR on optim.Adam: the reference's value exactly
        norm = check_norm(opt, grad_norm, g, N_GRAD)
        torch_norm = float(Z[f"{case}{it}_norm"])
        assert abs(float(grad_norm) - torch_norm) <= abs(torch_norm - norm) + 2.0 ** -23 * norm  # eval_util.py's rule
        p, g2, m, v, steps, _ = ou.step_f32(p, g, m, v, steps, lr, cfg["wd"], cfg["grad_clip"])
        out.append((read(opt, params), (p, g2, m, v, steps), g))
    return out


@pytest.mark.parametrize("case", list(ou.CASES))
def test_gpu_fused_step_is_bitwise_the_restatement(case):
    cfg = ou.CASES[case]
    for it, (got, want, g_in) in enumerate(run_case(case)):
        for a, b, what in zip(got[:4], want[:4], "pgmv"):
            same(a, b, f"{case}{it} {what}")
        assert got[4] == want[4] == [cfg["step0"] + (it + 1) * (g is not None) for g in g_in]
        assert got[4] == Z[f"{case}{it}_steps"].tolist()
        clipped = ou.clip_coef(ou.norm64(g_in)[0], cfg["grad_clip"]) != F(1.0)
        assert clipped == (case in "bd")
        for a, b in zip(got[1], g_in):  # (a), (c), (e): g untouched; (b), (d): scaled
            assert a is None or np.array_equal(a, b) != clipped


def sampled_iteration(case, it):
    """Iteration ``it`` alone on the device from TORCH's state after iteration ``it - 1`` at the fixture's sampled
    elements: one tensor per fixture tensor (its samples) and a last one whose gradient holds every element
    that is not sampled, so that the norm and the clip coefficient are those of the whole set.  Returns
    (device (p, g, m, v, steps), inputs (p, g, m, v), lr, coef)."""
    cfg = ou.CASES[case]
    key, prev = f"{case}{it}", f"{case}{it - 1}"
    lr = float(Z[key + "_lr"])
    grads = ou.gradients(case, it)
    idx = [ou.sample_indices(n) for n in ou.SIZES]
    p0, m0, v0, s0 = ou.initial_state(case)
    p, m, v, steps, g, rest = [], [], [], [], [], []
    for i, n in enumerate(ou.SIZES):
        if it == 0:
            p.append(p0[i][idx[i]]), m.append(m0[i][idx[i]]), v.append(v0[i][idx[i]]), steps.append(s0[i])
        else:
            has = f"{prev}_m{i}" in Z
            p.append(Z[f"{prev}_p{i}"]), steps.append(int(Z[prev + "_steps"][i]))
            m.append(Z[f"{prev}_m{i}"] if has else None), v.append(Z[f"{prev}_v{i}"] if has else None)
        if grads[i] is None:
            g.append(None)
        else:
            g.append(grads[i][idx[i]])
            rest.append(np.delete(grads[i], idx[i]))
    rest = np.concatenate(rest)
    opt, params = make_adam(p + [np.zeros(rest.size, F)], m + [None], v + [None], steps + [0], lr, views=())
    set_grads(params, g + [rest])
    grad_norm, _ = opt.step_fused(cfg["wd"], cfg["grad_clip"])
    norm = check_norm(opt, grad_norm, grads, N_GRAD)
    got = read(opt, params)
    return tuple(x[:-1] for x in got), (p, g, m, v), lr, ou.clip_coef(norm, cfg["grad_clip"])


@pytest.mark.parametrize("it", range(ou.ITERATIONS))
@pytest.mark.parametrize("case", list(ou.CASES))
def test_gpu_each_iteration_against_the_reference_run(case, it):
    cfg = ou.CASES[case]
    key = f"{case}{it}"
    got, inputs, lr, coef = sampled_iteration(case, it)
    assert got[4] == Z[key + "_steps"].tolist()
    worst = dict(m=0.0, v=0.0, p=0.0)
    for i in range(len(ou.SIZES)):
        if inputs[1][i] is None:
            assert np.array_equal(got[0][i], Z[f"{key}_p{i}"]) and got[4][i] == cfg["step0"]
            continue
        x = tuple(a[i] for a in inputs)
        if x[2] is None:
            x = (x[0], x[1], np.zeros_like(x[0]), np.zeros_like(x[0]))
        r = ou.ratios((got[0][i], got[2][i], got[3][i]), tuple(Z[f"{key}_{a}{i}"] for a in "pmv"), *x, lr, cfg["wd"],
                      coef, got[4][i])
        for k in worst:
            worst[k] = max(worst[k], r[k])
    print(f"{key}: device against torch, units of 2^-24: " + ", ".join(f"k_{k} {x:.3f}" for k, x in worst.items()))
    for k in worst:
        assert worst[k] <= ou.K[k], (k, worst[k])


@pytest.mark.parametrize("case", ["b", "e"])
def test_gpu_fused_equals_the_three_calls(case):
    """weight_decay(); check_update(); optimizer.step() on a copy: bitwise the fused result over three iterations,
    the returned norm and current_lr included ((b) clips, (e) has a decay that moves p)."""
    gu = load_pkg("generic_utils")
    cfg = ou.CASES[case]
    state = ou.initial_state(case)
    fused, fp = make_adam(*state, cfg["lr"])
    plain, pp = make_adam(*state, cfg["lr"])
    for it in range(ou.ITERATIONS):
        g = ou.gradients(case, it)
        set_grads(fp, g)
        set_grads(pp, g)
        norm_f, lr_f = fused.step_fused(cfg["wd"], cfg["grad_clip"])
        same_opt, lr_p = gu.weight_decay(plain, cfg["wd"])
        norm_p, skip = gu.check_update(pp, cfg["grad_clip"])
        plain.step()
        assert same_opt is plain and lr_p == lr_f == cfg["lr"] and skip is False
        assert torch.equal(norm_f, norm_p) and norm_p.shape == () and norm_p.is_cuda
        a, b = read(fused, fp), read(plain, pp)
        for x, y, what in zip(a[:4], b[:4], "pgmv"):
            same(x, y, f"{case}{it} {what}")
        assert a[4] == b[4]
    want = run_case(case)[-1][0]
    for x, y in zip(read(plain, pp)[:4], want[:4]):
        same(x, y)


def test_gpu_check_update_takes_a_module():
    gu = load_pkg("generic_utils")
    lin = torch.nn.Linear(5, 3).cuda()
    for P in lin.parameters():
        P.grad = torch.full_like(P, 2.0)
    w = lin.weight.detach().clone()
    grad_norm, skip = gu.check_update(lin, 1.0)
    assert skip is False and float(grad_norm) == F(np.sqrt(18 * 4.0))
    coef = ou.clip_coef(np.sqrt(72.0), 1.0)
    assert torch.equal(lin.weight.grad, torch.full_like(w, 2.0) * float(coef)) and torch.equal(lin.weight, w)
    opt = torch.optim.SGD(lin.parameters(), lr=0.5)  # any torch optimizer: weight_decay reads param_groups only
    _, lr = gu.weight_decay(opt, 0.25)
    assert lr == 0.5 and torch.equal(lin.weight, w + (-0.125) * w)  # (exact in float32)


def test_gpu_scalar_and_vector_paths_agree():
    """The same tensor as a view at element offset 1 (4-byte aligned: single floats) and as an aligned copy
    (16-byte moves), several chunks and a partial last quad: bitwise equal, clip and decay active."""
    g = np.random.Generator(np.random.PCG64(5))
    n = 2 * ou.CHUNK + 5
    p, m = (0.1 * g.standard_normal(n)).astype(F), (1e-3 * g.standard_normal(n)).astype(F)
    v, gr = (1e-4 * g.uniform(0.2, 1.0, n)).astype(F), (1e-2 * g.standard_normal(n)).astype(F)
    opt, params = make_adam([p, p], [m, m], [v, v], [7, 7], 1e-3, views=(0,))
    assert params[0].data_ptr() % 16 == 4 and params[1].data_ptr() % 16 == 0
    set_grads(params, [gr, gr])
    opt.step_fused(5e-2, 0.5)
    got = read(opt, params)
    for a, what in zip(got[:4], "pgmv"):
        same([a[0]], [a[1]], what)
    want = ou.step_f32([p, p], [gr, gr], [m, m], [v, v], [7, 7], 1e-3, 5e-2, 0.5)
    for a, b in zip(got[:4], want[:4]):
        same(a, b)
    assert not np.array_equal(got[1][0], gr)  # clipped


def test_gpu_tensor_without_gradient_and_one_element_tensor():
    got, want, g_in = run_case("d")[0]
    p, m, v, steps = ou.initial_state("d")
    assert g_in[ou.NONE] is None and got[4][ou.NONE] == 1000 and got[4][0] == 1001
    for a, b in zip((got[0], got[2], got[3]), (p, m, v)):  # bit-identical before and after
        same([a[ou.NONE]], [b[ou.NONE]])
    assert got[1][ou.NONE] is None
    # the 1-element tensor alone: one chunk, one lane
    g = [np.array([0.25], F)]
    opt, params = make_adam([np.array([-0.5], F)], [None], [None], [0], 1e-3, views=())
    set_grads(params, g)
    grad_norm, _ = opt.step_fused(5e-2, 0.125)
    assert float(opt.last_norm64) == 0.25 and float(grad_norm) == 0.25
    want = ou.step_f32([np.array([-0.5], F)], g, [np.zeros(1, F)], [np.zeros(1, F)], [0], 1e-3, 5e-2, 0.125)
    for a, b in zip(read(opt, params)[:4], want[:4]):
        same(a, b)


def test_gpu_repeated_iteration_reproduces_every_bit():
    cfg = ou.CASES["b"]
    runs = []
    for _ in range(2):
        opt, params = make_adam(*ou.initial_state("b"), cfg["lr"])
        set_grads(params, ou.gradients("b", 0))
        grad_norm, _ = opt.step_fused(cfg["wd"], cfg["grad_clip"])
        runs.append(read(opt, params) + (np.float64(float(opt.last_norm64)), grad_norm.cpu().numpy()))
    for a, b in zip(runs[0][:4], runs[1][:4]):
        same(a, b)
    assert runs[0][5].tobytes() == runs[1][5].tobytes() and runs[0][6].tobytes() == runs[1][6].tobytes()
    same(runs[0][0], run_case("b")[0][0][0])  # and the run of the first test, whose gradients lay elsewhere


def test_gpu_nonfinite_gradient():
    """The only test that feeds a non-finite value: ordinary arithmetic (max_norm / inf = 0, inf * 0 = NaN)."""
    cfg = ou.CASES["a"]
    g = ou.gradients("a", 0)
    g[4] = g[4].copy()
    g[4][17] = np.inf
    state = ou.initial_state("a")
    opt, params = make_adam(*state, cfg["lr"])
    set_grads(params, g)
    before = read(opt, params)
    grad_norm, lr, skip = opt.step_fused(cfg["wd"], cfg["grad_clip"], skip_nonfinite=True)
    after = read(opt, params)
    assert skip is True and lr == cfg["lr"] and np.isinf(opt.last_norm) and np.isinf(float(grad_norm))
    for a, b in zip(before[:4], after[:4]):
        same(a, b)
    assert after[4] == before[4] == [0] * len(ou.SIZES) and not opt.state_dict()["state"]
    grad_norm, lr = opt.step_fused(cfg["wd"], cfg["grad_clip"])  # not skipped: as torch's arithmetic goes
    got = read(opt, params)
    want = ou.step_f32(*state[:1], g, *state[1:], cfg["lr"], cfg["wd"], cfg["grad_clip"])
    assert np.isinf(want[5]) and np.isinf(float(grad_norm)) and np.isinf(float(opt.last_norm64))
    for a, b, what in zip(got[:4], want[:4], "pgmv"):
        for i, (x, y) in enumerate(zip(a, b)):
            if x is None:  # no gradient, no state: the restatement carries zeros there
                assert y is None or not np.any(y), (what, i)
            else:
                assert np.array_equal(x, y, equal_nan=True), (what, i)
    assert np.isnan(got[1][4][17]) and np.isnan(got[0][4][17]) and not np.isnan(got[0][4][16])
    assert not np.any(got[1][3]) and got[4] == want[4]  # every finite gradient times the coefficient 0
    # a finite norm with skip_nonfinite: the step is taken, the third value is False
    opt, params = make_adam(*state, cfg["lr"])
    set_grads(params, ou.gradients("a", 0))
    grad_norm, lr, skip = opt.step_fused(cfg["wd"], cfg["grad_clip"], skip_nonfinite=True)
    assert skip is False and opt.last_norm == float(opt.last_norm64)
    for a, b in zip(read(opt, params)[:4], run_case("a")[0][0][:4]):
        same(a, b)


def test_gpu_state_dict_round_trip_with_torch_adam():
    """After two steps the state loads into torch.optim.Adam and back.  A third step by each from that state:
    both results lie within K64 of the fp64 evaluation of the same inputs, m' and v' at every element, p' at the
    fixture's sampled elements, the population K64's constants were measured on.

    Why through the fp64 evaluation and not one float32 result against the other: torch's GPU kernels compute in
    their own order, and two float32 p' that differ by u |dp| before the last sum fall a whole ulp of p' apart
    wherever a rounding boundary lies between them.  Measured on an MI355X, device against torch's GPU Adam in
    the units of p's bound: 7523 over all elements and 52 / 396 at the sampled ones (cases (a) / (b)), while
    each side is within 0.8 / 2.1 of the fp64 evaluation there.  Over all 110 970 elements p's unit u |dp| itself
    is too small where m' cancels (dp is proportional to m', whose error is bounded by |m| + |g|, not by |m'|):
    101 and 130 for the device, 101 and 26 for torch, the same element leading in case (a)."""
    optim = load_pkg("optim")
    got2, _, _ = run_case("a")[1]
    p, _, m, v, steps = got2
    opt, params = make_adam(p, [x if x is not None else np.zeros(1, F) for x in m],
                            [x if x is not None else np.zeros(1, F) for x in v], steps, 1e-3)
    tparams = make_params(p)
    topt = torch.optim.Adam(tparams, lr=1e-3, betas=ou.BETAS, eps=ou.EPS, weight_decay=0)
    # (deep copies, as a checkpoint holds: load_state_dict keeps the very step tensors it is given)
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))
    back = optim.Adam(make_params(p), lr=1e-3, betas=ou.BETAS, eps=ou.EPS)
    back.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert [int(s["step"]) for s in back.state_dict()["state"].values()] == [s for s in steps if s]
    g = ou.gradients("a", 2)
    set_grads(params, g)
    set_grads(tparams, g)
    opt.step()
    topt.step()
    ours, theirs = read(opt, params), read(topt, tparams)
    assert ours[4] == theirs[4] == [s + 1 if s else 0 for s in steps]
    for name, res in (("device", ours), ("torch", theirs)):
        worst = dict(m=0.0, v=0.0, p=0.0)
        for i in range(len(ou.SIZES)):
            if g[i] is None:
                same([res[0][i]], [p[i]])
                continue
            for keys, ix in (("mv", np.arange(ou.SIZES[i])), ("p", ou.sample_indices(ou.SIZES[i]))):
                x = (p[i][ix], g[i][ix], m[i][ix], v[i][ix])
                e = ou.element_f64(*x, 1e-3, 0.0, F(1.0), steps[i] + 1)
                r = ou.ratios((res[0][i][ix], res[2][i][ix], res[3][i][ix]), (e[0], e[2], e[3]), *x, 1e-3, 0.0, F(1.0),
                              steps[i] + 1)
                for k in keys:
                    worst[k] = max(worst[k], r[k])
        print(f"third step, {name} against the fp64 evaluation, units of 2^-24: "
              + ", ".join(f"k_{k} {x:.3f}" for k, x in worst.items()))
        for k in worst:
            assert worst[k] <= ou.K64[k], (name, k, worst[k])


def test_gpu_stopnet_pair():
    """train.py:157-167: the model's optimizer over every tensor, a second one over the stopnet's two alone
    (a [1, 37] weight and a [1] bias stand in), clipped at 1.0, sharing the tensors: bitwise the restatement."""
    optim = load_pkg("optim")
    g = np.random.Generator(np.random.PCG64(11))
    shapes = [(300,), (1, 37), (1,)]
    p = [(0.1 * g.standard_normal(s)).astype(F) for s in shapes]
    g1 = [(1e-2 * g.standard_normal(s)).astype(F) for s in shapes]
    g2 = [(g.standard_normal(s)).astype(F) for s in shapes[1:]]  # norm ~ 6: the clip at 1.0 acts
    params = [torch.nn.Parameter(dev(a)) for a in p]
    opt = optim.Adam(params, lr=1e-3)
    opt_st = optim.Adam(params[1:], lr=1e-3)
    wd, grad_clip = 5e-2, 1e3
    set_grads(params, g1)
    opt.step_fused(wd, grad_clip)
    for P, x in zip(params[1:], g2):  # stop_loss.backward() adds to the gradients the first update left
        P.grad += dev(x)
    grad_norm_st, _ = opt_st.step_fused(wd, 1.0)
    flat = lambda xs: [x.reshape(-1) for x in xs]
    zeros = lambda xs: [np.zeros(x.size, F) for x in xs]
    p1, g1c, m1, v1, s1, _ = ou.step_f32(flat(p), flat(g1), zeros(p), zeros(p), [0, 0, 0], 1e-3, wd, grad_clip)
    gsum = [a + b.reshape(-1) for a, b in zip(g1c[1:], g2)]
    p2, g2c, m2, v2, s2, norm = ou.step_f32(p1[1:], gsum, zeros(p[1:]), zeros(p[1:]), [0, 0], 1e-3, wd, 1.0)
    assert ou.clip_coef(norm, 1.0) < F(0.5) and float(grad_norm_st) == F(float(opt_st.last_norm64))
    assert abs(float(opt_st.last_norm64) - norm) <= ou.norm_bound(38) * norm
    got, got_st = read(opt, params), read(opt_st, params[1:])
    same(flat(got[0]), [p1[0]] + p2), same(flat(got[1]), [g1c[0]] + g2c)
    same(flat(got[2]), m1), same(flat(got[3]), v1)      # the model optimizer's own state: one step
    same(flat(got_st[2]), m2), same(flat(got_st[3]), v2)
    assert got[4] == [1, 1, 1] and got_st[4] == [1, 1]


def test_gpu_argument_checks():
    native = load_pkg("_native")
    lib = native.lib()
    h = ctypes.c_void_p()
    native.check(lib.tts_optim_create(ctypes.byref(h)), "tts_optim_create")
    n = 2
    sizes = (5, ou.CHUNK + 3)
    t = {k: [torch.full((s,), val, device="cuda") for s in sizes] for k, val in (("p", 1.0), ("g", 2.0), ("m", 3.0), ("v", 4.0))}
    n64 = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    n32 = torch.full((2,), 7.0, device="cuda")
    host = dict(sumsq=ctypes.c_double(7.0), norm=ctypes.c_double(7.0))
    s = native.stream_handle()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    I64 = ctypes.c_int64

    def table(numel=sizes, step=(1, 1), **null):
        arr = (native.OptimTensor * n)()
        for i in range(n):
            for k in "pgmv":
                setattr(arr[i], k, None if null.get(k) == i else t[k][i].data_ptr())
            arr[i].numel, arr[i].step = numel[i], step[i]
        if null.get("same_p"):
            arr[1].p = arr[0].p
        return arr

    def call(name, h_=h, tab="default", n_=n, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, max_norm=1.0, n64_=ptr(n64),
             n32_=ptr(n32), **kw):
        tab = table(**kw) if tab == "default" else tab
        norm_args = (max_norm, n64_, n32_, ctypes.byref(host["sumsq"]), ctypes.byref(host["norm"]), s)
        args = dict(grad_norm=norm_args, clip=norm_args, decay=(lr, wd, s), adam=(lr, b1, b2, eps, s),
                    step=(lr, b1, b2, eps, wd, max_norm, n64_, n32_, s))[name]
        native.check(getattr(lib, "tts_optim_" + name)(h_, tab, n_, *args), "tts_optim_" + name)

    every = ("grad_norm", "clip", "decay", "adam", "step")
    with pytest.raises(RuntimeError, match="set_tensors"):
        call("step")  # before the sizes are set
    for bad, match in ((dict(h_=None), "null"), (dict(numel_=None), "null"), (dict(n_=0), "positive"),
                       (dict(sizes_=(5, 0)), "positive"), (dict(sizes_=(-1, 3)), "positive")):
        sz = bad.pop("sizes_", sizes)
        arr = None if "numel_" in bad else (I64 * n)(*sz)
        with pytest.raises(RuntimeError, match=match):
            native.check(lib.tts_optim_set_tensors(bad.get("h_", h), arr, bad.get("n_", n), s), "tts_optim_set_tensors")
    native.check(lib.tts_optim_set_tensors(h, (I64 * n)(*sizes), n, s), "tts_optim_set_tensors")
    for name in every:
        for bad, match in ((dict(h_=None), "null"), (dict(tab=None), "null"), (dict(n_=0), "positive"), (dict(n_=1), "sizes"),
                           (dict(numel=(5, 0)), "positive"), (dict(numel=(-5, ou.CHUNK + 3)), "positive"),
                           (dict(numel=(5, ou.CHUNK + 2)), "sizes"), (dict(p=1), "null p"), (dict(same_p=True), "same p")):
            with pytest.raises(RuntimeError, match=match):
                call(name, **bad)
    for name in ("grad_norm", "clip", "step"):
        for bad, match in ((dict(max_norm=0.0), "max_norm"), (dict(max_norm=-1.0), "max_norm"), (dict(n64_=None), "null"),
                           (dict(n32_=None), "null")):
            with pytest.raises(RuntimeError, match=match):
                call(name, **bad)
    for name in ("decay", "adam", "step"):
        for bad in (dict(lr=0.0), dict(lr=-1e-3)):
            with pytest.raises(RuntimeError, match="lr"):
                call(name, **bad)
    for name in ("adam", "step"):
        for bad, match in ((dict(b1=1.0), "beta"), (dict(b1=-0.1), "beta"), (dict(b2=1.0), "beta"), (dict(eps=-1e-8), "eps"),
                           (dict(m=0), "null m or v"), (dict(v=1), "null m or v"), (dict(step=(0, 1)), "below 1")):
            with pytest.raises(RuntimeError, match=match):
                call(name, **bad)
    torch.cuda.synchronize()
    for k, val in (("p", 1.0), ("g", 2.0), ("m", 3.0), ("v", 4.0)):  # nothing was launched
        assert all(bool((x == val).all()) for x in t[k])
    assert n64.tolist() == [7.0, 7.0] and n32.tolist() == [7.0, 7.0] and [x.value for x in host.values()] == [7.0, 7.0]
    call("grad_norm", max_norm=50.0)  # the same arguments, valid
    total = 4.0 * sum(sizes)  # (every partial is an integer: the sum is exact)
    assert n64.tolist() == [x.value for x in host.values()] and n64[0] == total
    assert abs(float(n64[1]) - np.sqrt(total)) <= 2.0 ** -52 * np.sqrt(total)
    assert n32.tolist() == [F(float(n64[1])), F(50.0 / (float(n64[1]) + 1e-6))] and bool((t["g"][1] == 2.0).all())
    call("decay", g=0, m=0, v=1, lr=0.5, wd=0.25)  # g, m, v are not read
    assert all(bool((x == 0.875).all()) for x in t["p"])
    call("adam", g=0)  # a tensor without a gradient needs no state and no step
    assert bool((t["p"][0] == 0.875).all()) and bool((t["m"][0] == 3.0).all()) and not bool((t["p"][1] == 0.875).any())
    native.check(lib.tts_optim_set_tensors(h, (I64 * n)(5, 6), n, s), "tts_optim_set_tensors")  # other sizes: rebuilt
    with pytest.raises(RuntimeError, match="sizes"):
        call("clip")
    lib.tts_optim_destroy(h)


def test_gpu_five_training_steps_on_a_small_mlp():
    """tests/test_tacotron2_model.py:21-69 of the reference, made small: five steps on a random target, every
    parameter changes, the loss after step 5 is below the loss before step 1."""
    optim = load_pkg("optim")
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, 8)).cuda()
    x, y = torch.randn(64, 16, device="cuda"), torch.randn(64, 8, device="cuda")
    before = [P.detach().clone() for P in model.parameters()]
    opt = optim.Adam(model.parameters(), lr=1e-2)
    crit = torch.nn.MSELoss()
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = crit(model(x), y)
        loss.backward()
        grad_norm, lr = opt.step_fused(1e-6, 1.0)
        losses.append(float(loss.detach()))
        assert lr == 1e-2 and float(grad_norm) > 0.0
    losses.append(float(crit(model(x), y).detach()))
    print("losses", losses)
    assert losses[-1] < losses[0]
    for P, b in zip(model.parameters(), before):
        assert bool((P != b).any())
    assert all(int(s["step"]) == 5 for s in opt.state.values())
