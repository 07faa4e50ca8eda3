"""GPU: layers.GRU (tts_gru_forward / tts_gru_backward, csrc/gru_train.hip) against the float64 restatement of
tests/gru_train_util.py and the gru_train.npz fixture (the reference's GRU modules with autograd), under the bound
of gru_train_util.py; determinism, the two upstream gradients, reserve ownership, no_grad / eval, stale weights, a
strided input, the C ABI's NULL gradients and INVALID cases, and one train.train_batch iteration of a
Tacotron-shaped model through use_device_gru.

Measured on an MI355X: the worst figure in the bound's form over these cases is 1.1e-6 against the bound of 4e-6, and
3.5e-8 in the swap test (tools/bench_gru_train.py writes them per case into profiles/gru_train.json, "device_errors").
"""
import ctypes

import numpy as np
import pytest
import torch

import gru_train_util as gu
import train_util as tu
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu


def make_module(inp):
    layers = load_pkg("layers")
    m = layers.GRU(inp["I"], inp["H"], batch_first=True, bidirectional=inp["bi"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
    return m.cuda().train()


def cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


def run(case, m=None, x_grad=True, zeros_for_missing=False, x=None):
    """Forward and backward of a case -> {tensor name: numpy array} (grad_x missing without ``x_grad``).  With
    ``zeros_for_missing`` an upstream gradient the case lacks is passed as zeros instead of being left out."""
    inp = gu.inputs(case)
    m = m or make_module(inp)
    x = (cuda(inp["x"]) if x is None else x).requires_grad_(x_grad)
    out, h_n = m(x, cuda(inp["h0"]))
    ups = {"out": (out, cuda(inp["up_out"])), "h_n": (h_n, cuda(inp["up_hn"]))}
    if zeros_for_missing:
        ups = {k: (t, torch.zeros_like(t) if u is None else u) for k, (t, u) in ups.items()}
    ups = [(t, u) for t, u in ups.values() if u is not None]
    params = dict(m.named_parameters())
    grads = torch.autograd.grad([t for t, _ in ups], ([x] if x_grad else []) + list(params.values()), [u for _, u in ups])
    r = {"out": out, "h_n": h_n}
    r.update(zip((["grad_x"] if x_grad else []) + ["grad_" + n for n in params], grads))
    return {k: v.detach().cpu().numpy() for k, v in r.items()}


_cache, _restated = {}, {}


def result(case):
    if case not in _cache:
        _cache[case] = run(case)
    return _cache[case]


def restated(case):
    if case not in _restated:
        _restated[case] = gu.restate(gu.inputs(case))
    return _restated[case]


@pytest.fixture(scope="module")
def fixture():
    return golden("gru_train")


def bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", list(gu.CASES))
def test_within_the_bound_of_restatement_and_fixture(case, fixture):
    got, ref = result(case), restated(case)
    ref32 = gu.reference_fp32(fixture)
    names = gu.tensor_names(gu.CASES[case]["bi"])
    assert sorted(got) == sorted(names)
    for name in names:
        assert got[name].dtype == np.float32 and got[name].shape == ref[name].shape
        tol = gu.tolerance(ref32, case, name)
        gu.check(got[name], ref[name], f"{case} {name} vs restatement", tol)
        gu.check(gu.stored(case, name, got[name]), fixture[gu.key(case, name, 64)], f"{case} {name} vs fixture", tol,
                 scale=np.abs(ref[name]).max())


def test_deterministic():
    a, b = run("t24"), run("t24")
    for name in a:
        assert bitwise(a[name], b[name]), name


@pytest.mark.parametrize("case", ["t3", "gst"])  # grad_out only; grad_h_n only
def test_a_missing_upstream_is_zeros(case):
    alone, with_zeros = result(case), run(case, zeros_for_missing=True)
    for name in alone:
        assert bitwise(alone[name], with_zeros[name]), name


def test_no_grad_eval_and_nothing_requiring_grad_keep_no_reserve():
    inp = gu.inputs("t3")
    m = make_module(inp)
    x = cuda(inp["x"])
    out_train, hn_train = m(x)
    assert m.last_reserve_floats == 2 * 3 * 2 * 128 * 4 and out_train.requires_grad and hn_train.requires_grad
    with torch.no_grad():
        out_ng, hn_ng = m(x)
    assert m.last_reserve_floats == 0 and not out_ng.requires_grad
    m(x)
    assert m.last_reserve_floats > 0
    m.eval()
    out_eval, hn_eval = m(x)
    assert m.last_reserve_floats == 0
    m.train()
    m(x)
    assert m.last_reserve_floats > 0
    for p in m.parameters():
        p.requires_grad_(False)
    out_frozen, hn_frozen = m(x)
    assert m.last_reserve_floats == 0 and not out_frozen.requires_grad
    for o, h in ((out_ng, hn_ng), (out_eval, hn_eval), (out_frozen, hn_frozen)):
        assert bitwise(o.cpu().numpy(), out_train.detach().cpu().numpy())
        assert bitwise(h.cpu().numpy(), hn_train.detach().cpu().numpy())


def test_reserve_belongs_to_the_call():
    """Two forwards on different inputs, then both backwards: each gets its own gradients."""
    ia, ib = gu.inputs("t3"), gu.inputs("t2")
    m = make_module(ia)
    params = list(m.parameters())

    def forward(inp):
        x = cuda(inp["x"]).requires_grad_(True)
        return x, m(x)[0], cuda(inp["up_out"])

    def backward(x, out, up):
        return [g.cpu().numpy() for g in torch.autograd.grad([out], [x] + params, [up])]

    one_a = backward(*forward(ia))
    one_b = backward(*forward(ib))
    fa, fb = forward(ia), forward(ib)
    both_a, both_b = backward(*fa), backward(*fb)
    for one, both in ((one_a, both_a), (one_b, both_b)):
        for g1, g2 in zip(one, both):
            assert bitwise(g1, g2)
    assert not bitwise(one_a[1], one_b[1])


def test_weights_follow_the_optimizer_and_load_state_dict():
    layers, optim = load_pkg("layers"), load_pkg("optim")
    inp = gu.inputs("small")
    m = make_module(inp)
    opt = optim.Adam(m.parameters(), lr=0.01)
    x, up = cuda(inp["x"]), cuda(inp["up_out"])
    before = m(x)[0]
    assert m.repacks == 1
    before.backward(up)
    opt.step()
    after = m(x)[0]
    assert m.repacks == 2
    fresh = layers.GRU(inp["I"], inp["H"], batch_first=True, bidirectional=True).cuda()
    fresh.load_state_dict(m.state_dict())
    want = fresh(x)[0]
    assert bitwise(after.detach().cpu().numpy(), want.detach().cpu().numpy())
    assert not bitwise(after.detach().cpu().numpy(), before.detach().cpu().numpy())
    m(x)
    with torch.no_grad():
        m(x)
    assert m.repacks == 2
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
    again = m(x)[0]
    assert m.repacks == 3
    assert bitwise(again.detach().cpu().numpy(), before.detach().cpu().numpy())


def test_parameters_modified_between_forward_and_backward_raise():
    inp = gu.inputs("t2")
    m = make_module(inp)
    out = m(cuda(inp["x"]))[0]
    with torch.no_grad():
        m.bias_hh_l0.add_(1.0)
    with pytest.raises(RuntimeError, match="modified"):
        out.backward(cuda(inp["up_out"]))


def test_a_transposed_offset_view_of_x_gives_the_bits_of_its_copy():
    inp = gu.inputs("t24")
    B, T, I = inp["x"].shape
    base = torch.zeros(T, B, I + 3, device="cuda")
    view = base[:, :, 1:1 + I].transpose(0, 1)  # [B, T, I]: strided, 4 bytes off a 16-byte boundary
    view.copy_(cuda(inp["x"]))
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    got = run("t24", x=view.detach())
    for name, want in result("t24").items():
        assert bitwise(got[name], want), name


def test_hx_that_requires_grad_raises_and_a_packed_sequence_is_not_implemented():
    inp = gu.inputs("state")
    m = make_module(inp)
    x = cuda(inp["x"])
    with pytest.raises(NotImplementedError):
        m(x, cuda(inp["h0"]).requires_grad_(True))
    with pytest.raises(NotImplementedError):
        m(torch.nn.utils.rnn.pack_padded_sequence(x, [5, 5], batch_first=True))


def test_c_abi_null_gradients_and_invalid_calls():
    n = load_pkg("_native")
    inp = gu.inputs("small")
    m = make_module(inp)
    full = result("small")
    x, up = cuda(inp["x"]), cuda(inp["up_out"])
    lib, h = m._handle()
    m._sync_weights()
    B, T, _ = x.shape
    D, H = 2, inp["H"]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    out = torch.full((B, T, D * H), 7.0, device="cuda")
    reserve = torch.empty(lib.tts_gru_reserve_floats(h, B, T), device="cuda")
    s = n.stream_handle()

    def forward(B=B, T=T, x=x, out=out, reserve=reserve):
        return lib.tts_gru_forward(h, p(x), B, T, None, p(out), None, p(reserve), s)

    assert forward(B=0) == 1 and forward(T=0) == 1 and forward(x=None) == 1 and forward(out=None) == 1
    assert forward(B=1 << 12, T=1 << 12) == 1  # B * T >= 2^24
    assert forward(x=x.view(-1)[1:]) == 1      # misaligned
    fresh = ctypes.c_void_p()
    assert lib.tts_gru_create(inp["I"], H, 1, ctypes.byref(fresh)) == 0
    assert lib.tts_gru_forward(fresh, p(x), B, T, None, p(out), None, None, s) == 1  # weights not set
    lib.tts_gru_destroy(fresh)
    for bad in ((inp["I"], 144), (24, 48), (0, 48), (32, 0)):
        assert lib.tts_gru_create(bad[0], bad[1], 1, ctypes.byref(fresh)) == 3  # TTS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a rejected call wrote its output"
    assert forward() == 0
    assert bitwise(out.cpu().numpy(), full["out"])

    names = gu.param_names(True)
    grads = {k: torch.full(tuple(v.shape), 7.0, device="cuda") for k, v in inp["weights"].items()}
    grad_x = torch.full_like(x, 7.0)

    def pair(kind, skip=()):
        arr = (ctypes.c_void_p * 2)()
        for d, sfx in enumerate(("", "_reverse")):
            name = kind + sfx
            arr[d] = None if name in skip else grads[name].data_ptr()
        return arr

    def backward(skip=(), gx=grad_x, up=up, ghn=None, reserve=reserve, out=out):
        return lib.tts_gru_backward(h, p(x), B, T, p(reserve), p(out), None, p(up), p(ghn), p(gx),
                                    *[pair(k, skip) for k in gu.PARAMS], s)

    assert backward(up=None) == 1, "grad_out and grad_h_n both NULL"
    assert backward(reserve=None) == 1 and backward(out=None) == 1
    assert backward(up=up.view(-1)[1:]) == 1
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in list(grads.values()) + [grad_x]), "a rejected call wrote a gradient"
    skip = ("weight_hh_l0", "bias_ih_l0_reverse", "weight_ih_l0_reverse")
    assert backward(skip=skip, gx=None) == 0
    torch.cuda.synchronize()
    assert bool((grad_x == 7.0).all())
    for name in names:
        got = grads[name].cpu().numpy()
        if name in skip:
            assert (got == 7.0).all(), f"{name}: a NULL gradient's product was written somewhere"
        else:
            assert bitwise(got, full["grad_" + name]), name
    assert backward() == 0
    assert bitwise(grad_x.cpu().numpy(), full["grad_x"])
    for name in names:
        assert bitwise(grads[name].cpu().numpy(), full["grad_" + name]), name


def test_train_batch_through_use_device_gru(fixture):
    """The util's Tacotron-shaped model through train.train_batch, once as torch and once after use_device_gru: the
    losses, every parameter's gradient and the parameters after the step within the bound of a float64 CPU run of
    the same torch model (plain SGD on both sides: gru_train_util.torch_train_step says why)."""
    layers, train = load_pkg("layers"), load_pkg("train")
    c = tu.config("TacotronGST", grad_clip=1e9)  # a clip coefficient of exactly 1
    ref = gu.torch_train_step(gu.tiny_model(), c, torch.float64)
    ref32 = gu.reference_fp32(fixture)

    def step(swap):
        model = gu.tiny_model().cuda().train()
        if swap:
            assert layers.use_device_gru(model) is model
            assert [type(model.get_submodule(path)) for path, *_ in gu.SITES] == [layers.GRU] * 3
        opt = torch.optim.SGD(model.parameters(), lr=gu.SWAP_LR)
        opt_st = torch.optim.SGD(model.decoder.stopnet.parameters(), lr=gu.SWAP_LR)
        out = train.train_batch(model, c, tu.batch("cuda"), opt, opt_st)
        return out, model

    for swap in (False, True):
        what = "device GRU" if swap else "torch"
        out, model = step(swap)
        for k, v in ref["losses"].items():
            gu.check(np.float64(out[k]), np.float64(v), f"{what} {k}", gu.tolerance(ref32, "swap", k))
        params = dict(model.named_parameters())
        assert sorted(params) == sorted(ref["grads"])
        for name, p in params.items():
            gu.check(p.grad.cpu().numpy(), ref["grads"][name], f"{what} grad {name}",
                     gu.tolerance(ref32, "swap", "grads." + name))
            gu.check(p.detach().cpu().numpy(), ref["params"][name], f"{what} stepped {name}",
                     gu.tolerance(ref32, "swap", "params." + name))
        if swap:
            assert all(model.get_submodule(path).repacks == 1 for path, *_ in gu.SITES)


def test_a_batch_whose_grids_pass_65535_workgroups():
    """B = 16 * 65536 + 1, T = 1: the loop kernels need more than 65535 sentence tiles and the input projection and
    grad_x more than 65535 row blocks, so neither may sit on grid.y.  out, h_n and grad_x (per-row quantities) are
    held to the bound; the last sentence is the one live row of the last tile."""
    case = dict(seed=541, I=16, H=16, bi=True, B=16 * 65536 + 1, T=1)
    inp = gu.inputs(case)
    m = make_module(inp)
    for p in m.parameters():
        p.requires_grad_(False)
    x = cuda(inp["x"]).requires_grad_(True)
    out, h_n = m(x)
    (grad_x,) = torch.autograd.grad([out], [x], [cuda(inp["up_out"])])
    ref = gu.restate(inp)
    for name, got in (("out", out), ("h_n", h_n), ("grad_x", grad_x)):
        gu.check(got.detach().cpu().numpy(), ref[name], f"large batch {name}")
