"""The trainable decoder on the device (layers.Decoder over tts_dectrain_*): every case of decoder_train_util.py
within the bound of the float64 restatement and of the reference's float64 run (tests/golden/decoder_train.npz),
then the contract: padding, determinism, the reserve, weights, masks, the swap, train_batch, the C ABI.

Measured on an MI355X (profiles/decoder_train.json, "device_errors"): the worst figure over the cases is 2.7e-6
(grad_attention_rnn.weight_ih of "chunks", 576 rows summed), the forward's outputs are at or below 2.1e-6."""
import ctypes
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import decoder_train_util as du  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "decoder_train.npz"))


def load_pkg(name):
    return importlib.import_module("your-voice-tts_amd." + name)


def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_module(case, inp=None):
    c, inp = du.case_of(case), inp or du.inputs(case)
    d = c["dims"]
    m = load_pkg("layers").Decoder(d["E"], d["mel"], c["r"], False, c["norm"], "original", c["pdrop"], c["fwd"], False,
                                   False, False, c["sep"], prenet_dim=d["PN"], rnn_dim=d["R"], attention_dim=d["A"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
    return m.cuda().train(c["training"])


def device_masks(inp):
    return None if inp["masks"] is None else {k: torch.from_numpy(v).cuda() for k, v in inp["masks"].items()}


def run(case, m=None, inp=None, grads=(True, True), backward=True):
    """Forward (and backward with the case's upstream gradients) on the device: {name: numpy array}."""
    c, inp = du.case_of(case), inp or du.inputs(case)
    m = m or make_module(case, inp)
    x = torch.from_numpy(inp["inputs"]).cuda().requires_grad_(grads[0] and c["training"])
    mem = torch.from_numpy(inp["memories"]).cuda().requires_grad_(grads[1] and c["training"])
    m.zero_grad()
    o, s, a = m(x, mem, torch.from_numpy(inp["mask"]).cuda(), device_masks(inp))
    got = {"outputs": o, "stop_tokens": s, "alignments": a}
    if c["training"] and backward:
        up = inp["up"]
        ((o * torch.from_numpy(up["outputs"]).cuda()).sum() + (s * torch.from_numpy(up["stop_tokens"]).cuda()).sum()).backward()
        if x.grad is not None:
            got["grad_inputs"] = x.grad
        if mem.grad is not None:
            got["grad_memories"] = mem.grad
        for n, p in m.named_parameters():
            got["grad_" + n] = p.grad
    return {k: v.detach().cpu().numpy() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def result(case):
    return run(case)


@pytest.mark.parametrize("case", list(du.CASES))
def test_case_within_the_bound(case):
    got, ref = result(case), du.restated(case)
    for name in du.tensor_names(case):
        scale = du.scale_of(case, name, ref)
        du.check(got[name], ref[name], f"{case} {name} vs the restatement", du.TOL, scale)
        if case in du.FIXTURE_CASES:
            tol = du.tolerance({case: {name: float(GOLD[du.key(case, name, "ref32")])}}, case, name)
            du.check(du.stored(case, name, got[name]), GOLD[du.key(case, name, 64)], f"{case} {name} vs the reference",
                     tol, scale)


def test_padding():
    inp = dict(du.inputs("t6"))
    poisoned = inp["inputs"].copy()
    poisoned[inp["mask"] == 0] = np.nan
    got, want = run("t6", inp=dict(inp, inputs=poisoned)), result("t6")
    for name in du.tensor_names("t6"):
        assert bitwise(got[name], want[name]), name
    g = got["grad_inputs"][inp["mask"] == 0]
    assert g.size and np.array_equal(g.view(np.uint32), np.zeros(g.shape, np.uint32)), "grad_inputs is not +0.0 on masked rows"


def test_deterministic():
    a, b = run("r2_fwd"), result("r2_fwd")
    for name in du.tensor_names("r2_fwd"):
        assert bitwise(a[name], b[name]), name


def _forward(m, inp, **kw):
    x = torch.from_numpy(inp["inputs"]).cuda().requires_grad_(kw.get("grad", True))
    mem = torch.from_numpy(inp["memories"]).cuda()
    return x, m(x, mem, torch.from_numpy(inp["mask"]).cuda(), kw.get("masks", device_masks(inp)))


def test_reserve_belongs_to_the_call():
    inp, inp2 = du.inputs("t6"), du.inputs("nodrop")
    m = make_module("t6")
    x1, (o1, s1, _) = _forward(m, inp)
    x2, (o2, s2, _) = _forward(m, dict(inp, inputs=inp2["inputs"]))  # a second forward before the first backward
    up = torch.from_numpy(inp["up"]["outputs"]).cuda()
    (o2 * up).sum().backward()
    (o1 * up).sum().backward()
    m2 = make_module("t6")
    x3, (o3, _, _) = _forward(m2, inp)
    (o3 * up).sum().backward()
    assert bitwise(x1.grad.cpu().numpy(), x3.grad.cpu().numpy())
    assert not bitwise(x1.grad.cpu().numpy(), x2.grad.cpu().numpy())


def test_no_grad_and_eval_keep_no_reserve():
    inp = du.inputs("t6")
    m = make_module("t6")
    _, (o, s, a) = _forward(m, inp)
    assert m.last_reserve_floats > 0 and o.requires_grad and s.requires_grad and not a.requires_grad
    with torch.no_grad():
        _, (o_ng, s_ng, a_ng) = _forward(m, inp)
    assert m.last_reserve_floats == 0 and not o_ng.requires_grad
    for p in m.parameters():
        p.requires_grad_(False)
    _, (o_c, s_c, a_c) = _forward(m, inp, grad=False)
    assert m.last_reserve_floats == 0
    for got, want in ((o_ng, o), (s_ng, s), (a_ng, a), (o_c, o), (s_c, s), (a_c, a)):
        assert bitwise(got.cpu().numpy(), want.detach().cpu().numpy())
    m.eval()
    _forward(m, inp, grad=False)
    assert m.last_reserve_floats == 0 and m.last_masks is None


def test_weights_follow_the_optimizer_and_are_not_repacked_without_need():
    optim = load_pkg("optim")
    inp = du.inputs("small")
    m = make_module("small")
    opt = optim.Adam(m.parameters(), lr=0.01)
    _, (before, _, _) = _forward(m, inp)
    assert m.repacks == 1
    before.sum().backward()
    opt.step()
    _, (after, _, _) = _forward(m, inp)
    assert m.repacks == 2
    fresh = make_module("small")
    fresh.load_state_dict(m.state_dict())
    _, (want, _, _) = _forward(fresh, inp)
    assert bitwise(after.detach().cpu().numpy(), want.detach().cpu().numpy())
    assert not bitwise(after.detach().cpu().numpy(), before.detach().cpu().numpy())
    _forward(m, inp)
    with torch.no_grad():
        _forward(m, inp)
    assert m.repacks == 2
    # a parameter changed between a forward and its backward
    _, (o, _, _) = _forward(m, inp)
    with torch.no_grad():
        m.decoder_rnn.bias_ih.add_(1.0)
    with pytest.raises(RuntimeError, match="modified"):
        o.sum().backward()


def test_needs_input_grad():
    full = result("small")
    for grads, absent in (((False, True), "grad_inputs"), ((True, False), "grad_memories")):
        got = run("small", grads=grads)
        assert absent not in got
        for name in got:
            assert bitwise(got[name], full[name]), name


def test_seeded_masks():
    inp = du.inputs("small")
    m = make_module("small")
    outs = []
    for _ in range(2):
        torch.manual_seed(77)
        _, (o, s, _) = _forward(m, inp, masks=None)
        outs.append((o.detach().cpu().numpy(), s.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in m.last_masks.items()}))
    assert set(outs[0][2]) == {"prenet", "att", "dec", "stop"}
    for k in outs[0][2]:
        assert np.array_equal(outs[0][2][k], outs[1][2][k]) and 0 < outs[0][2][k].mean() < 1
    assert bitwise(outs[0][0], outs[1][0]) and bitwise(outs[0][1], outs[1][1])


def test_use_device_decoder():
    layers = load_pkg("layers")
    inp = du.inputs("small")

    class Model(torch.nn.Module):
        pass

    model = Model()
    model.decoder = old = du.torch_decoder("small", inp["weights"]).cuda().train()
    assert layers.use_device_decoder(model) is model
    new = model.decoder
    assert isinstance(new, layers.Decoder) and new.training and next(new.parameters()).is_cuda
    assert list(new.state_dict()) == list(old.state_dict())
    for k, v in old.state_dict().items():
        assert torch.equal(v, new.state_dict()[k]), k
    layers.use_device_decoder(model)
    assert model.decoder is new  # idempotent
    args = (torch.from_numpy(inp["inputs"]).cuda(), torch.from_numpy(inp["memories"]).cuda(),
            torch.from_numpy(inp["mask"]).cuda(), device_masks(inp))
    ref = du.restated("small")
    with torch.no_grad():
        for dec, what in ((new, "swapped"), (old, "torch")):
            o, s, a = dec(*args)
            for name, t in (("outputs", o), ("stop_tokens", s), ("alignments", a)):
                du.check(t.cpu().numpy(), ref[name], f"{what} {name}")
    new.eval()
    model.decoder = du.torch_decoder("small", inp["weights"]).cuda().eval()
    assert not layers.use_device_decoder(model).decoder.training


@pytest.mark.parametrize("separate", [True, False])
def test_train_batch_all_layers(separate):
    import train_util as tu
    layers, optim, train = load_pkg("layers"), load_pkg("optim"), load_pkg("train")
    c = tu.config(separate_stopnet=separate, r=du.MODEL_R)
    model = du.small_model(separate).cuda().train()
    layers.use_device_decoder(layers.use_device_convs(layers.use_device_lstm(model)))
    dec = model.decoder
    assert isinstance(dec, layers.Decoder) and isinstance(model.encoder.lstm, layers.LSTM)
    assert all(isinstance(b, layers.ConvBNBlock) for b in list(model.encoder.convolutions) + list(model.postnet.convolutions))
    start = {k: v.detach().cpu().numpy().copy() for k, v in dec.named_parameters()}
    opt = optim.Adam(model.parameters(), lr=c.lr, weight_decay=0)
    opt_st = optim.Adam(dec.stopnet.parameters(), lr=c.lr, weight_decay=0) if separate else None
    iterations = 3
    for _ in range(iterations):
        out = train.train_batch(model, c, du.model_batch("cuda"), opt, opt_st)
        assert all(np.isfinite(out[k]) for k in ("loss", "decoder_loss", "postnet_loss", "stop_loss"))
        for name, p in dec.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), name
    assert dec.repacks == iterations
    for name, p in dec.named_parameters():
        assert not np.array_equal(p.detach().cpu().numpy(), start[name]), f"{name} did not move"


def test_c_abi_rejects_bad_arguments_before_any_launch():
    n = load_pkg("_native")
    inp = du.inputs("small")
    m = make_module("small")
    x, (good, good_stop, _) = _forward(m, inp, grad=False)
    good = good.detach().transpose(1, 2).contiguous()  # [B, T * r, mel] = the C layout [B][T][MR]
    lib, h = m._handle()
    B, L, T = x.shape[0], x.shape[1], du.CASES["small"]["T"]
    mem, text_mask = torch.from_numpy(inp["memories"]).cuda(), torch.from_numpy(inp["mask"]).cuda()
    out, stop = torch.full_like(good, 7.0), torch.full((B, T), 7.0, device="cuda")
    align = torch.full((B, T, L), 7.0, device="cuda")
    dm = device_masks(inp)  # (kept alive: the tables hold raw pointers)
    table = m._mask_table(dm)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def forward(x=x, mem=mem, B=B, L=L, T=T, training=1, table=table, out=out, stop=stop, align=align, h=h, reserve=None):
        return lib.tts_dectrain_forward(h, P(x), P(mem), P(text_mask), B, L, T, training,
                                        ctypes.byref(table) if table is not None else None, P(out), P(stop), P(align),
                                        reserve, n.stream_handle())

    assert forward(x=None) == 1 and forward(mem=None) == 1 and forward(out=None) == 1 and forward(stop=None) == 1
    assert forward(align=None) == 1 and forward(h=None) == 1
    assert forward(B=0) == 1 and forward(L=0) == 1 and forward(T=0) == 1 and forward(table=None) == 1
    broken = m._mask_table(dm)
    broken.att_c = None
    assert forward(table=broken) == 1
    broken = m._mask_table(dm)
    broken.scale_rnn = 0.0
    assert forward(table=broken) == 1
    room = torch.empty(lib.tts_dectrain_reserve_floats(h, B, L, T) + 4, dtype=torch.float32, device="cuda")
    assert room.data_ptr() % 16 == 0 and forward(reserve=ctypes.c_void_p(room.data_ptr() + 4)) == 1  # misaligned reserve
    grads = n.DectrainTensors()
    assert lib.tts_dectrain_backward(h, P(text_mask), B, L, T, ctypes.byref(table), ctypes.c_void_p(room.data_ptr() + 4),
                                     P(out), None, None, None, ctypes.byref(grads), n.stream_handle()) == 1
    assert lib.tts_dectrain_backward(h, None, B, L, T, ctypes.byref(table), None, P(out), None, None, None,
                                     ctypes.byref(grads), n.stream_handle()) == 1  # no reserve
    fresh = ctypes.c_void_p()
    assert lib.tts_dectrain_create(32, 16, 40, 16, 24, 0, 1, 1, 1, ctypes.byref(fresh)) != 0  # rnn no multiple of 16
    assert lib.tts_dectrain_create(32, 16, 48, 16, 24, 2, 1, 1, 1, ctypes.byref(fresh)) == 1  # unknown norm
    assert lib.tts_dectrain_create(32, 16, 48, 16, 24, 0, 1, 1, 1, ctypes.byref(fresh)) == 0
    assert forward(h=fresh) == 1  # weights not set
    lib.tts_dectrain_destroy(fresh)
    assert lib.tts_dectrain_reserve_floats(None, B, L, T) == 0 and lib.tts_dectrain_reserve_floats(h, 0, L, T) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stop == 7.0).all()) and bool((align == 7.0).all()), "a rejected call wrote"
    assert forward() == 0
    torch.cuda.synchronize()
    assert bitwise(out.cpu().numpy(), good.cpu().numpy()) and bitwise(stop.cpu().numpy(), good_stop.detach().cpu().numpy())
