"""GPU: layers.ConvBNBlock (tts_convbn_forward / tts_convbn_backward, csrc/convbn_train.hip) against the float64
restatement of tests/convbn_train_util.py and the convbn_train.npz fixture (the reference's ConvBNBlock,
Encoder.convolutions and Postnet.convolutions with autograd), under the bound of convbn_train_util.py; dropout
zeros, the mask, determinism, strided input, eval(), no_grad, reserve ownership, needs_input_grad, stale
parameters, repacks, one train.train_batch iteration through use_device_convs, and the C-ABI's rejections.

Measured on an MI355X (profiles/convbn_train.json, "device_errors"): the worst figure in the bound's form over these
cases is 1.9e-6 (grad_W of the second block of "postnet"), against the bound of 4e-6; 2.8e-6 at the training shapes.
"""
import ctypes

import numpy as np
import pytest
import torch

import convbn_train_util as cu
import train_util as tu
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return golden("convbn_train")


def make_blocks(inp):
    layers = load_pkg("layers")
    blocks = []
    for blk in inp["blocks"]:
        m = layers.ConvBNBlock(blk["cin"], blk["cout"], 5, blk["act"])
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cu.state_dict(blk).items()})
        blocks.append(m.cuda().train())
    return blocks


def forward(blocks, x, masks):
    for m, mask in zip(blocks, masks):
        x = m(x, None if mask is None else torch.from_numpy(mask).cuda())
    return x


def run(case, masks, blocks=None, x_grad=True, x=None):
    """Forward, backward and a second forward of a case -> {tensor name: numpy array}."""
    inp = cu.inputs(case)
    blocks = blocks or make_blocks(inp)
    if x is None:
        x = torch.from_numpy(inp["x"]).cuda()
    x = x.requires_grad_(x_grad)
    out = forward(blocks, x, masks)
    params = [p for m in blocks for p in m._params()]
    grads = torch.autograd.grad([out], ([x] if x_grad else []) + params, [torch.from_numpy(inp["up"]).cuda()])
    r = {"out": out}
    if x_grad:
        r["grad_x"], grads = grads[0], grads[1:]
    for i, m in enumerate(blocks):
        for j, p in enumerate(cu.PARAMS):
            r[f"grad_{p}{i}"] = grads[4 * i + j]
        r[f"rm1_{i}"], r[f"rv1_{i}"] = m.net[1].running_mean.clone(), m.net[1].running_var.clone()
    forward(blocks, x.detach(), masks)
    for i, m in enumerate(blocks):
        r[f"rm2_{i}"], r[f"rv2_{i}"] = m.net[1].running_mean.clone(), m.net[1].running_var.clone()
    r = {k: v.detach().cpu().numpy() for k, v in r.items()}
    r["num_batches_tracked"] = [int(m.net[1].num_batches_tracked) for m in blocks]
    return r


_cache, _restated = {}, {}


def result(case, fixture):
    if case not in _cache:
        _cache[case] = run(case, cu.masks(fixture, case))
    return _cache[case]


def restated(case, fixture):
    if case not in _restated:
        _restated[case] = cu.restate(cu.inputs(case), cu.masks(fixture, case))
    return _restated[case]


def bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_bits(a, b):
    for name in a:
        if name == "num_batches_tracked":
            assert a[name] == b[name]
        else:
            assert bitwise(a[name], b[name]), name


@pytest.mark.parametrize("case", list(cu.CASES))
def test_within_the_bound_of_restatement_and_fixture(case, fixture):
    got, ref = result(case, fixture), restated(case, fixture)
    names = cu.tensor_names(case)
    assert sorted(got) == sorted(names + ["num_batches_tracked"])
    for name in names:
        assert got[name].dtype == np.float32
        scale = cu.bias_scale(name, ref)
        cu.check(got[name], ref[name], f"{case} {name} vs restatement", scale)
        cu.check(cu.stored(case, name, got[name]), fixture[cu.key(case, name, 64)], f"{case} {name} vs fixture", scale)
    assert got["num_batches_tracked"] == fixture[cu.key(case, "num_batches_tracked", "i")].tolist()


@pytest.mark.parametrize("case", ["t3", "post_in", "post_out", "b17t19"])
def test_dropped_elements_are_positive_zero(case, fixture):
    mask = cu.masks(fixture, case)[-1]
    out = result(case, fixture)["out"]
    assert (mask == 0).any() and not out.view(np.uint32)[mask == 0].any()
    if cu.CASES[case]["blocks"][-1][2] != "relu":
        assert (out[mask != 0] != 0).all()


def test_a_given_mask_is_the_one_used(fixture):
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    m = make_blocks(inp)[0]
    x = torch.from_numpy(inp["x"]).cuda()
    out = m(x, torch.from_numpy(masks[0]).cuda())
    assert m.last_mask.dtype == torch.uint8 and np.array_equal(m.last_mask.cpu().numpy(), masks[0])
    as_bool = m(x, torch.from_numpy(masks[0]).bool())
    assert bitwise(out.detach().cpu().numpy(), as_bool.detach().cpu().numpy())
    flipped = m(x, torch.from_numpy(1 - masks[0]).cuda())
    assert np.array_equal(flipped.detach().cpu().numpy() != 0, masks[0] == 0)
    with pytest.raises(ValueError):
        m(x, torch.ones(3, 32, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        m(x, torch.ones(3, 32, 9))


def test_drawn_mask_follows_the_seed_and_keeps_half():
    inp = cu.inputs("post_in")
    x = torch.from_numpy(inp["x"]).cuda()
    outs, drawn = [], []
    for seed in (77, 77, 78):
        m = make_blocks(inp)[0]
        torch.manual_seed(seed)
        outs.append(m(x).detach().cpu().numpy())
        drawn.append(m.last_mask.cpu().numpy())
    assert np.array_equal(drawn[0], drawn[1]) and bitwise(outs[0], outs[1])
    assert not np.array_equal(drawn[0], drawn[2])
    n = drawn[0].size
    share = drawn[0].sum() / n
    print(f"kept share {share:.4f} of {n}")
    assert set(np.unique(drawn[0])) == {0, 1} and abs(share - 0.5) <= 2.5 / np.sqrt(n)  # five sigma, seed fixed
    assert np.array_equal(outs[0] != 0, drawn[0] != 0)  # (tanh: no kept element is zero)


@pytest.mark.parametrize("case", ["b17t19", "chunks"])
def test_deterministic(case, fixture):
    masks = cu.masks(fixture, case)
    same_bits(run(case, masks), run(case, masks))


@pytest.mark.parametrize("case", ["post_in", "small"])
def test_strided_input_gives_the_contiguous_bits(case, fixture):
    inp, masks = cu.inputs(case), cu.masks(fixture, case)
    want = result(case, fixture)
    x = torch.from_numpy(inp["x"]).cuda()
    transposed = x.transpose(1, 2).contiguous().transpose(1, 2)  # as embedding(text).transpose(1, 2)
    assert not transposed.is_contiguous()
    flat = torch.zeros(x.numel() + 3, device="cuda")
    flat[3:] = x.reshape(-1)
    offset = flat[3:].view(x.shape)  # at an odd float offset: 4-byte aligned only
    assert offset.data_ptr() % 16 != 0
    for view in (transposed, offset):
        same_bits(run(case, masks, x=view.detach()), want)


def test_eval_uses_the_running_statistics_and_keeps_nothing(fixture):
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    m = make_blocks(inp)[0]
    x = torch.from_numpy(inp["x"]).cuda()
    m(x, torch.from_numpy(masks[0]).cuda())  # the running statistics move off 0 and 1
    assert m.last_reserve_floats > 0
    rm, rv = m.net[1].running_mean.clone(), m.net[1].running_var.clone()
    m.eval()
    out = m(x)
    assert m.last_reserve_floats == 0 and m.last_mask is None and not out.requires_grad
    want, _, _, _ = cu.block_forward(inp["x"].astype(np.float64), inp["blocks"][0], None,
                                     rm.cpu().numpy().astype(np.float64), rv.cpu().numpy().astype(np.float64),
                                     training=False)
    cu.check(out.cpu().numpy(), want, "eval out")
    masked = m(x, torch.from_numpy(masks[0]).cuda())
    assert bitwise(masked.cpu().numpy(), out.cpu().numpy()), "eval() read the mask"
    assert torch.equal(m.net[1].running_mean, rm) and torch.equal(m.net[1].running_var, rv)
    assert int(m.net[1].num_batches_tracked) == 1


def test_no_grad_gives_the_training_bits_and_keeps_nothing(fixture):
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    mask = torch.from_numpy(masks[0]).cuda()
    x = torch.from_numpy(inp["x"]).cuda()
    a, b = make_blocks(inp)[0], make_blocks(inp)[0]
    out_train = a(x, mask)
    assert a.last_reserve_floats > 0 and out_train.requires_grad
    with torch.no_grad():
        out_ng = b(x, mask)
    assert b.last_reserve_floats == 0 and not out_ng.requires_grad
    assert bitwise(out_ng.cpu().numpy(), out_train.detach().cpu().numpy())
    for m in (a, b):
        assert int(m.net[1].num_batches_tracked) == 1
    assert torch.equal(a.net[1].running_mean, b.net[1].running_mean) and bool(a.net[1].running_mean.abs().max() > 0)
    assert torch.equal(a.net[1].running_var, b.net[1].running_var)
    for p in b.parameters():
        p.requires_grad_(False)
    assert not b(x, mask).requires_grad and b.last_reserve_floats == 0


def test_reserve_belongs_to_the_call(fixture):
    """Two forwards on different inputs, then both backwards: each gets its own gradients."""
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    m = make_blocks(inp)[0]
    mask = torch.from_numpy(masks[0]).cuda()
    xa = torch.from_numpy(inp["x"]).cuda()
    xb = torch.from_numpy(np.ascontiguousarray(inp["x"][::-1, :, ::-1])).cuda()
    up = torch.from_numpy(inp["up"]).cuda()

    def fwd(x):
        x = x.clone().requires_grad_(True)
        return x, m(x, mask)

    def bwd(x, out):
        return [g.cpu().numpy() for g in torch.autograd.grad([out], [x] + m._params(), [up])]

    one_a, one_b = bwd(*fwd(xa)), bwd(*fwd(xb))
    fa, fb = fwd(xa), fwd(xb)
    both_a, both_b = bwd(*fa), bwd(*fb)
    for one, both in ((one_a, both_a), (one_b, both_b)):
        for g1, g2 in zip(one, both):
            assert bitwise(g1, g2)
    assert not bitwise(one_a[1], one_b[1])


def test_needs_input_grad(fixture):
    masks = cu.masks(fixture, "small")
    full = result("small", fixture)
    got = run("small", masks, x_grad=False)
    assert "grad_x" not in got
    same_bits(got, full)
    inp = cu.inputs("small")
    m = make_blocks(inp)[0]
    x = torch.from_numpy(inp["x"]).cuda()
    m(x, torch.from_numpy(masks[0]).cuda()).backward(torch.from_numpy(inp["up"]).cuda())
    assert x.grad is None and bitwise(m.net[0].weight.grad.cpu().numpy(), full["grad_W0"])
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    x.requires_grad_(True)
    m(x, torch.from_numpy(masks[0]).cuda()).backward(torch.from_numpy(inp["up"]).cuda())
    assert bitwise(x.grad.cpu().numpy(), full["grad_x"]) and m.net[0].weight.grad is None


def test_a_parameter_changed_before_the_backward_raises(fixture):
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    m = make_blocks(inp)[0]
    out = m(torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(masks[0]).cuda())
    with torch.no_grad():
        m.net[1].weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified"):
        out.backward(torch.from_numpy(inp["up"]).cuda())


def test_weights_follow_the_optimizer_and_are_not_repacked_without_need(fixture):
    layers, optim = load_pkg("layers"), load_pkg("optim")
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    m = make_blocks(inp)[0]
    mask = torch.from_numpy(masks[0]).cuda()
    opt = optim.Adam(m.parameters(), lr=0.01)
    x, up = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["up"]).cuda()
    before = m(x, mask)
    assert m.repacks == 1
    before.backward(up)
    assert m.repacks == 1
    opt.step()
    stats = {k: v.clone() for k, v in m.state_dict().items()}
    after = m(x, mask)
    assert m.repacks == 2
    fresh = layers.ConvBNBlock(48, 32, 5, "tanh").cuda()
    fresh.load_state_dict(stats)
    want = fresh(x, mask)
    assert bitwise(after.detach().cpu().numpy(), want.detach().cpu().numpy())
    assert not bitwise(after.detach().cpu().numpy(), before.detach().cpu().numpy())
    m(x, mask)
    with torch.no_grad():
        m(x, mask)
    m.eval()(x)
    assert m.repacks == 2


def test_one_value_per_channel_in_training_raises():
    layers = load_pkg("layers")
    m = layers.ConvBNBlock(48, 32, 5, "tanh").cuda().train()
    with pytest.raises(ValueError):
        m(torch.zeros(1, 48, 1, device="cuda"))
    assert int(m.net[1].num_batches_tracked) == 0
    assert m.eval()(torch.zeros(1, 48, 1, device="cuda")).shape == (1, 32, 1)


def test_train_batch_through_use_device_convs():
    layers, optim, train = load_pkg("layers"), load_pkg("optim"), load_pkg("train")
    c = tu.config(grad_clip=1e9)  # a clip coefficient of exactly 1: the gradients stay as the backward wrote them
    model = cu.tiny_model()
    keys = list(model.state_dict())
    model = layers.use_device_lstm(layers.use_device_convs(model.cuda().train()))
    assert list(model.state_dict()) == keys
    blocks = {("encoder", i): b for i, b in enumerate(model.encoder.convolutions)}
    blocks.update({("postnet", i): b for i, b in enumerate(model.postnet.convolutions)})
    assert len(blocks) == 5 and all(isinstance(b, layers.ConvBNBlock) for b in blocks.values())
    assert isinstance(model.encoder.lstm, layers.LSTM)
    before = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    opt = optim.Adam(model.parameters(), lr=c.lr, weight_decay=0)
    opt_st = optim.Adam(model.decoder.stopnet.parameters(), lr=c.lr, weight_decay=0)
    out = train.train_batch(model, c, tu.batch("cuda"), opt, opt_st)
    assert np.isfinite(out["loss"])
    for (part, i), b in blocks.items():
        seen = {k: v.cpu().numpy() for k, v in model.seen[(part, i)].items()}
        prefix = f"{part}.convolutions.{i}."
        blk = dict(act=b.nonlinear, cin=b.in_channels, cout=b.out_channels,
                   **{p: before[prefix + cu.STATE_KEYS[p]] for p in cu.PARAMS})
        mask = b.last_mask.cpu().numpy()
        ref_out, saved, rm, rv = cu.block_forward(seen["x"].astype(np.float64), blk, mask,
                                                  before[prefix + "net.1.running_mean"].astype(np.float64),
                                                  before[prefix + "net.1.running_var"].astype(np.float64))
        _, grads, S = cu.block_backward(seen["grad_out"].astype(np.float64), blk, saved)
        cu.check(seen["out"], ref_out, f"train_batch {prefix}out")
        for p, t in zip(cu.PARAMS, b._params()):
            cu.check(t.grad.cpu().numpy(), grads[p], f"train_batch {prefix}grad_{p}", S if p == "bias" else None)
        cu.check(b.net[1].running_mean.cpu().numpy(), rm, f"train_batch {prefix}running_mean")
        cu.check(b.net[1].running_var.cpu().numpy(), rv, f"train_batch {prefix}running_var")
        assert int(b.net[1].num_batches_tracked) == 1
    after = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    for k in keys:
        assert not np.array_equal(after[k], before[k]), f"{k} did not move"


def test_c_abi_rejects_bad_arguments_before_any_launch(fixture):
    n = load_pkg("_native")
    inp, masks = cu.inputs("small"), cu.masks(fixture, "small")
    m = make_blocks(inp)[0]
    x = torch.from_numpy(inp["x"]).cuda()
    mask = torch.from_numpy(masks[0]).cuda()
    with torch.no_grad():
        good = m(x, mask).clone()
    lib, h = m._handle()
    B, _, T = x.shape
    out = torch.full_like(good, 7.0)
    rm, rv = torch.full((32,), 3.0, device="cuda"), torch.full((32,), 5.0, device="cuda")
    reserve = torch.full((lib.tts_convbn_reserve_floats(h, B, T),), 7.0, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(B=B, T=T, x=x, mask=mask, rm=rm, rv=rv, out=out, training=1):
        return lib.tts_convbn_forward(h, P(x), B, T, P(mask), 2.0, P(rm), P(rv), 0.1, 1e-5, training, P(out), P(reserve),
                                      n.stream_handle())

    assert call(B=0) == 1 and call(B=-1) == 1 and call(T=0) == 1
    assert call(B=1, T=1) == 1  # n == 1 in training
    assert call(x=None) == 1 and call(out=None) == 1
    assert call(mask=None) == 1 and call(rm=None) == 1 and call(rv=None) == 1
    gx = torch.full_like(x, 7.0)
    bwd = lambda **kw: lib.tts_convbn_backward(h, P(kw.get("x", x)), kw.get("B", B), T, P(kw.get("reserve", reserve)),
                                               P(kw.get("mask", mask)), P(kw.get("gout", good)), P(gx), None, None, None,
                                               None, n.stream_handle())
    assert bwd(B=0) == 1 and bwd(x=None) == 1 and bwd(reserve=None) == 1 and bwd(mask=None) == 1 and bwd(gout=None) == 1
    torch.cuda.synchronize()
    for t, v in ((out, 7.0), (reserve, 7.0), (gx, 7.0), (rm, 3.0), (rv, 5.0)):
        assert bool((t == v).all()), "a rejected call wrote"
    assert call(rm=m.net[1].running_mean.clone(), rv=m.net[1].running_var.clone()) == 0
    assert bitwise(out.cpu().numpy(), good.cpu().numpy())
