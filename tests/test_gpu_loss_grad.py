"""The criteria's gradient on the device (tts_loss_backward through losses.py and autograd) against the float64
restatement at every element and against the reference's own gradients at the stored ones (loss_grad.npz,
tests/golden/make_golden_loss_grad.py): every case and kind, masked and plain, upstream gradients 1 and 0.375;
the padding's +0.0, the NaN of an empty batch, the L1 tie, pitched operands whose padding is never read,
sentinels around a pitched grad_input, accumulation over two criteria, the calls that must stay outside
autograd, and the argument checks of the entry point.

Bounds (loss_grad_util.py): |got - g64| <= 2^-24 |g64| (1 + 2^-20); |got - ref32| <= |ref32 - ref64| + the same
of ref64; BCE adds 4 * 2^-53 |k| / n to both.  test_loss_grad_cpu.py shows that float32(g64) passes both.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eval_util as eu
import loss_grad_util as lg
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu
Z = golden("loss_grad")
inputs = functools.lru_cache(maxsize=None)(lg.inputs)


def _criterion(kind, name):
    lo = load_pkg("losses")
    return {("l1", "masked"): lo.L1LossMasked, ("mse", "masked"): lo.MSELossMasked, ("l1", "plain"): lo.L1Loss,
            ("mse", "plain"): lo.MSELoss}[kind, name]()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _backward(crit, x, y, lengths, k):
    """(loss, gradient) of k * crit(x, y[, lengths]) for a CUDA tensor x made a leaf here."""
    x = x.detach().requires_grad_()
    loss = crit(x, y, *(() if lengths is None else (lengths,)))
    assert loss.grad_fn is not None and loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    (loss if k == 1.0 else k * loss).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32 and x.grad.is_cuda
    return loss.detach(), x.grad


@pytest.mark.parametrize("k", lg.UPSTREAM)
@pytest.mark.parametrize("case,kind,name", lg.RUNS)
def test_gpu_elementwise_gradients(case, kind, name, k):
    x, y, lengths = inputs(case)
    lengths = lengths if name == "masked" else None
    crit = _criterion(kind, name)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    loss, grad = _backward(crit, xd, yd, None if lengths is None else torch.LongTensor(lengths), k)
    value = crit.last_value
    got = grad.cpu().numpy()
    g64 = lg.elementwise_grad(kind, x, y, lengths, k)
    key = lg.key(case, kind, name, k)
    lg.check_gradient(got, g64, what=key + " (every element)")
    lg.check_gradient(lg.stored(case, got), lg.stored(case, g64), Z[key + "_32"], Z[key + "_64"], what=key)
    if case == "d" and name == "masked":
        assert np.isnan(got).all() and np.isnan(value)
    else:
        pad = ~lg.valid_mask(x.shape, lengths)
        assert (got[pad] == 0).all() and not np.signbit(got[pad]).any()  # +0.0
        assert np.array_equal(got == 0, g64 == 0)
    if case == "g" and kind == "l1":
        tie = lg.ties("g")
        assert tie.any() and (got[tie] == 0).all() and not np.signbit(got[tie]).any()
    # the forward on the differentiable path is bitwise the evaluation's
    plain = crit(xd, yd, *(() if lengths is None else (lengths,)))
    assert plain.grad_fn is None and torch.equal(_bits(plain), _bits(loss))
    assert crit.last_value == value or (np.isnan(value) and np.isnan(crit.last_value))


@pytest.mark.parametrize("k", lg.UPSTREAM)
def test_gpu_bce_gradient(k):
    x, y = eu.bce_inputs()
    crit = load_pkg("losses").BCEWithLogitsLoss()
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    loss, grad = _backward(crit, xd, yd, None, k)
    value = crit.last_value
    key = f"e_bce_k{lg.UPSTREAM.index(k)}"
    lg.check_gradient(grad.cpu().numpy(), lg.bce_grad(x, y, k), Z[key + "_32"], Z[key + "_64"], lg.bce_abs(k, x.size),
                      what=key)
    assert torch.equal(_bits(crit(xd, yd)), _bits(loss)) and crit.last_value == value
    # [B, steps] logits, as the stop tokens come: the same gradient in that shape
    _, grad2 = _backward(crit, xd.view(1, -1), yd.view(1, -1), None, k)
    assert grad2.shape == (1, x.size) and torch.equal(_bits(grad2.view(-1)), _bits(grad))


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_gpu_padding_is_not_read_and_pitch_is_free(case, kind):
    """The operands inside larger pitched buffers at odd offsets, every padding row and every element between
    T * D and the pitch 1e30 in the input's and NaN in the target's; the input is the pitched view itself, and it
    requires grad: bitwise the contiguous gradient."""
    x, y, lengths = inputs(case)
    B, T, D = x.shape
    crit = _criterion(kind, "masked")
    want_loss, want = _backward(crit, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), lengths, 0.375)

    def embed(v, pitch, offset, fill):
        buf = torch.full((offset + B * pitch,), fill, device="cuda")
        view = buf[offset:].view(B, pitch)[:, :T * D].view(B, T, D)  # (a view: batch stride = pitch)
        for b in range(B):
            rows = min(lengths[b], T)
            view[b, :rows] = torch.from_numpy(v[b, :rows]).cuda()
        assert view.stride() == (pitch, D, 1) and view.data_ptr() == buf.data_ptr() + 4 * offset
        return view

    for (px, ox), (py, oy) in (((T * D + 3, 1), (T * D + 6, 2)), ((T * D, 0), (2 * T * D + 1, 3))):
        xv = embed(x, px, ox, 1e30).requires_grad_()
        loss = crit(xv, embed(y, py, oy, float("nan")), lengths)
        (0.375 * loss).backward()
        assert xv.grad.shape == (B, T, D) and torch.equal(_bits(xv.grad), _bits(want)), (px, ox, py, oy)
        assert torch.equal(_bits(loss), _bits(want_loss))


def _raw(native, kind, x, xp, y, yp, n_valid, B, per, count, gout, grad, gp):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    native.check(native.lib().tts_loss_backward(kind, p(x), xp, p(y), yp, p(n_valid), B, per, count, p(gout), p(grad),
                                                gp, native.stream_handle()), "tts_loss_backward")


@pytest.mark.parametrize("case", ["g", "h"])
def test_gpu_grad_pitch_leaves_the_gaps_alone(case):
    """The entry point itself, grad_input pre-filled with a sentinel and grad_pitch > T * D: the elements between
    T * D and the pitch and behind the last sentence keep the sentinel; the rest is the criterion's gradient."""
    native = load_pkg("_native")
    x, y, lengths = inputs(case)
    B, T, D = x.shape
    per, gp, tail = T * D, T * D + 5, 9
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    _, want = _backward(_criterion("mse", "masked"), xd, yd, lengths, 0.375)
    n_valid = torch.tensor([min(n, T) * D for n in lengths], dtype=torch.int64).cuda()
    buf = torch.full((B * gp + tail,), 7.0, device="cuda")
    gout = torch.tensor(0.375, device="cuda")
    _raw(native, native.TTS_LOSS_MSE, xd, per, yd, per, n_valid, B, per, int(n_valid.sum()), gout, buf, gp)
    rows = buf[:B * gp].view(B, gp)
    assert torch.equal(_bits(rows[:, :per]), _bits(want.view(B, per)))
    assert bool((rows[:, per:] == 7.0).all()) and bool((buf[B * gp:] == 7.0).all())
    # no table and no upstream gradient: every element valid, grad_output 1
    buf.fill_(7.0)
    _raw(native, native.TTS_LOSS_L1, xd, per, yd, per, None, B, per, B * per, None, buf, gp)
    _, want = _backward(_criterion("l1", "plain"), xd, yd, None, 1.0)
    assert torch.equal(_bits(rows[:, :per]), _bits(want.view(B, per)))
    assert bool((rows[:, per:] == 7.0).all()) and bool((buf[B * gp:] == 7.0).all())


def test_gpu_two_criteria_accumulate_on_one_input():
    """(dec + post).backward() with one input tensor under both criteria: .grad is the sum of the two single
    gradients as torch adds them."""
    x, y, lengths = inputs("g")
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    y2 = yd.flip(0).contiguous()
    crit = _criterion("mse", "masked")
    _, g1 = _backward(crit, xd, yd, lengths, 1.0)
    _, g2 = _backward(crit, xd, y2, lengths, 1.0)
    xt = xd.clone().requires_grad_()
    (crit(xt, yd, lengths) + crit(xt, y2, lengths)).backward()
    assert torch.equal(_bits(xt.grad), _bits(g1 + g2))
    # through an op of torch's in front of the criterion: the chain rule reaches the leaf
    w = torch.full((x.shape[2],), 0.5, device="cuda", requires_grad=True)
    crit(xd * w, yd, lengths).backward()
    terms = _backward(crit, xd * 0.5, yd, lengths, 1.0)[1].double() * xd.double()
    n = x.shape[0] * x.shape[1]  # a float32 sum of n rounded products, in torch's order
    assert bool(((w.grad.double() - terms.sum((0, 1))).abs() <= n * 2.0 ** -23 * terms.abs().sum((0, 1))).all())
    assert bool((w.grad != 0).all())


def test_gpu_calls_that_stay_outside_autograd():
    x, y, lengths = inputs("h")
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    lo = load_pkg("losses")
    for crit, args in ((lo.L1LossMasked(), (lengths,)), (lo.MSELoss(), ()), (lo.BCEWithLogitsLoss(), ())):
        out = crit(xd, yd, *args)  # does not require grad
        assert out.grad_fn is None and not out.requires_grad
        with torch.no_grad():
            out = crit(xd.clone().requires_grad_(), yd, *args)
        assert out.grad_fn is None and not out.requires_grad
        # a differentiable input is used as it is: no silent conversion that would cut the graph
        with pytest.raises(ValueError, match="CUDA float32"):
            crit(torch.from_numpy(x).requires_grad_(), yd, *args)
        with pytest.raises(ValueError, match="CUDA float32"):
            crit(xd.double().requires_grad_(), yd, *args)
        # the target gets no gradient, and a second backward through the same graph is torch's usual error
        xt, yt = xd.clone().requires_grad_(), yd.clone().requires_grad_()
        loss = crit(xt, yt, *args)
        loss.backward()
        assert yt.grad is None and xt.grad is not None
        with pytest.raises(RuntimeError, match="second time"):
            loss.backward()
    torch.cuda.synchronize()


def test_gpu_backward_argument_checks():
    native = load_pkg("_native")
    B, T, D = 2, 3, 5
    per = T * D
    x = torch.ones(B, T, D, device="cuda")
    y = torch.zeros(B, T, D, device="cuda")
    grad = torch.full((B, per), 7.0, device="cuda")
    n_valid = torch.tensor([per, per], dtype=torch.int64).cuda()

    def call(kind=native.TTS_LOSS_L1, x_=x, xp=per, y_=y, yp=per, B_=B, per_=per, count=B * per, grad_=grad, gp=per):
        _raw(native, kind, x_, xp, y_, yp, n_valid, B_, per_, count, None, grad_, gp)

    for bad in (dict(x_=None), dict(y_=None), dict(grad_=None)):
        with pytest.raises(RuntimeError, match="null"):
            call(**bad)
    for bad in (dict(B_=0), dict(per_=0), dict(per_=-1)):
        with pytest.raises(RuntimeError, match="positive"):
            call(**bad)
    for bad in (dict(xp=per - 1), dict(yp=per - 1), dict(gp=per - 1)):
        with pytest.raises(RuntimeError, match="pitch"):
            call(**bad)
    with pytest.raises(RuntimeError, match="negative"):
        call(count=-1)
    for kind in (-1, 3):
        with pytest.raises(RuntimeError, match="kind"):
            call(kind=kind)
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())  # nothing was launched
    call()  # the same arguments, valid
    assert bool((grad == np.float32(1.0 / 30.0)).all())
