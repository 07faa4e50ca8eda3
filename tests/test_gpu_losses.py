"""The device losses (tts_loss_masked, tts_loss_bce_logits through losses.py) against the reference's own
values (eval.npz, tests/golden/make_golden_eval.py), cases (a) to (e) of the fixture; padding that is never
read, pitched operands, repeatability, and the argument checks of both entry points.

Bounds (eval_util.py): the fp64 value and the per-sentence sums lie within (N + 4) * 2^-52 relative of the
fixture's float64 values, N the number of terms; the float32 scalar is the fp64 value rounded once, and its
distance to the reference's float32 value is at most |ref32 - ref64| + 2^-23 |ref64|, both from the fixture.
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_util as eu
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu
Z = golden("eval")
ELEMENTWISE = [(case, kind, name) for case, (_, _, lengths) in eu.LOSS_CASES.items() for kind in ("l1", "mse")
               for name in (("plain", "masked") if lengths is not None else ("plain",))]


def _criterion(kind, name):
    lo = load_pkg("losses")
    return {("l1", "masked"): lo.L1LossMasked, ("mse", "masked"): lo.MSELossMasked, ("l1", "plain"): lo.L1Loss,
            ("mse", "plain"): lo.MSELoss}[kind, name]()


def _check_scalar(out, crit, key):
    ref64, ref32 = float(Z[key + "_64"]), float(Z[key + "_32"])
    assert out.shape == () and out.dtype == torch.float32 and out.is_cuda
    got32 = out.cpu().numpy()
    if np.isnan(ref64):
        assert np.isnan(crit.last_value) and np.isnan(got32)
        return
    n = int(Z[key + "_count"])
    print(f"{key}: value {crit.last_value!r} ref64 {ref64!r} rel err {abs(crit.last_value - ref64) / abs(ref64):.3e} "
          f"bound {eu.fp64_bound(n):.3e}; f32 {got32!r} ref32 {ref32!r}")
    assert eu.within(crit.last_value, ref64, n)
    assert got32 == np.float32(crit.last_value)
    assert abs(float(got32) - ref32) <= abs(ref32 - ref64) + 2.0 ** -23 * abs(ref64)


@pytest.mark.parametrize("case,kind,name", ELEMENTWISE)
def test_gpu_elementwise_losses(case, kind, name):
    x, y, lengths = eu.loss_inputs(case)
    masked = name == "masked"
    crit = _criterion(kind, name)
    args = (torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) + ((torch.LongTensor(lengths),) if masked else ())
    out = crit(*args)
    key = f"{case}_{kind}_{name}"
    _check_scalar(out, crit, key)
    assert crit.last_count == int(Z[key + "_count"])
    per = crit.last_per_sentence
    assert per.shape == (x.shape[0],) and per.dtype == torch.float64 and per.is_cuda
    for b, (got, ref) in enumerate(zip(per.cpu().numpy(), Z[key + "_per"])):
        assert eu.within(got, ref, eu.sentence_terms(x.shape, lengths if masked else None, b)), b
    if masked:  # the lengths as a list, and a repeated call: bitwise the same three outputs
        first = (out.clone(), crit.last_value, crit.last_sum, per.clone())
        again = crit(args[0], args[1], list(lengths))
        assert torch.equal(again, first[0]) or (torch.isnan(again) and torch.isnan(first[0]))
        assert np.array_equal([crit.last_value, crit.last_sum], first[1:3], equal_nan=True)
        assert torch.equal(crit.last_per_sentence, first[3])


def test_gpu_bce_with_logits():
    x, y = eu.bce_inputs()
    crit = load_pkg("losses").BCEWithLogitsLoss()
    out = crit(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    _check_scalar(out, crit, "e_bce")
    assert np.isfinite(crit.last_value) and crit.last_count == 257
    assert eu.within(float(crit.last_per_sentence.cpu()[0]) / 257, float(Z["e_bce_64"]), 257)
    first = (out.clone(), crit.last_value, crit.last_sum)
    again = crit(torch.from_numpy(x).cuda().view(1, -1), torch.from_numpy(y).cuda().view(1, -1))  # [B, steps] logits
    assert torch.equal(again, first[0]) and (crit.last_value, crit.last_sum) == first[1:]


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_gpu_padding_is_not_read_and_pitch_is_free(case, kind):
    """The same operands inside larger pitched buffers, at other base alignments, every padding row and every
    element between T * D and the pitch 1e30 (and NaN in the target's): bitwise the contiguous result."""
    x, y, lengths = eu.loss_inputs(case)
    B, T, D = x.shape
    crit = _criterion(kind, "masked")
    want = crit(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), lengths).clone()
    want_value, want_sum, want_per = crit.last_value, crit.last_sum, crit.last_per_sentence.clone()

    def embed(v, pitch, offset, fill):
        buf = torch.full((offset + B * pitch,), fill, device="cuda")
        view = buf[offset:].view(B, pitch)[:, :T * D].view(B, T, D)  # (a view: batch stride = pitch)
        for b in range(B):
            rows = min(lengths[b], T)
            view[b, :rows] = torch.from_numpy(v[b, :rows]).cuda()
        assert view.stride() == (pitch, D, 1) and view.data_ptr() == buf.data_ptr() + 4 * offset
        return view

    for (px, ox), (py, oy) in (((T * D + 3, 1), (T * D + 6, 2)), ((T * D, 0), (2 * T * D + 1, 3))):
        got = crit(embed(x, px, ox, 1e30), embed(y, py, oy, float("nan")), lengths)
        assert torch.equal(got, want), (px, ox, py, oy)
        assert crit.last_value == want_value and crit.last_sum == want_sum
        assert torch.equal(crit.last_per_sentence, want_per)


def test_gpu_one_long_sentence_many_chunks():
    """One sentence of many 8192-element chunks whose last is partial, next to two short ones (one chunk each,
    no chunk for the empty one): the fold over more partials than a wave has lanes."""
    B, T, D = 4, 700, 1025
    lengths = [3, 700, 0, 1]
    g = np.random.Generator(np.random.PCG64(7))
    x = g.standard_normal((B, T, D)).astype(np.float32)
    y = g.standard_normal((B, T, D)).astype(np.float32)
    crit = _criterion("l1", "masked")
    out = crit(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), lengths)
    ref, count, per = eu.elementwise_loss("l1", x, y, lengths)
    assert crit.last_count == count == 704 * 1025
    assert eu.within(crit.last_value, ref, count) and out.cpu().numpy() == np.float32(crit.last_value)
    for b in range(B):
        assert eu.within(float(crit.last_per_sentence[b]), per[b], eu.sentence_terms(x.shape, lengths, b)), b


def test_gpu_batch_pitch_past_2_31():
    """Sentence 1 of the input starts more than 2^31 elements behind sentence 0 (an 8 GiB allocation that is
    touched only where the two sentences lie): bitwise the contiguous result."""
    x, y, lengths = eu.loss_inputs("a")
    x, y, lengths = x[:2], y[:2], [13, 5]
    crit = _criterion("mse", "masked")
    want = crit(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), lengths).clone()
    want_per = crit.last_per_sentence.clone()
    T, D = x.shape[1:]
    pitch = 2 ** 31 + 4
    buf = torch.empty(pitch + T * D, device="cuda")
    view = buf.as_strided((2, T, D), (pitch, D, 1))
    view.copy_(torch.from_numpy(x))
    got = crit(view, torch.from_numpy(y).cuda(), lengths)
    assert torch.equal(got, want) and torch.equal(crit.last_per_sentence, want_per)


def test_gpu_argument_checks():
    native = load_pkg("_native")
    lib = native.lib()
    h = ctypes.c_void_p()
    native.check(lib.tts_loss_create(ctypes.byref(h)), "tts_loss_create")
    B, T, D = 2, 3, 5
    x = torch.ones(B, T, D, device="cuda")
    y = torch.zeros(B, T, D, device="cuda")
    per = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    loss = torch.full((), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    host = dict(total=ctypes.c_double(7.0), count=ctypes.c_int64(7), value=ctypes.c_double(7.0))
    s = native.stream_handle()

    def masked(h_=h, kind=0, x_=p(x), xp=T * D, y_=p(y), yp=T * D, lens=(3, 3), B_=B, T_=T, D_=D, per_=p(per),
               loss_=p(loss), total=ctypes.byref(host["total"]), count=ctypes.byref(host["count"]),
               value=ctypes.byref(host["value"])):
        lens = native.i32_array(lens) if lens is not None else None
        native.check(lib.tts_loss_masked(h_, kind, x_, xp, y_, yp, lens, B_, T_, D_, per_, loss_, total, count, value,
                                         s), "tts_loss_masked")

    def bce(h_=h, x_=p(x), y_=p(y), n=B * T * D, per_=p(per), loss_=p(loss), total=ctypes.byref(host["total"]),
            value=ctypes.byref(host["value"])):
        native.check(lib.tts_loss_bce_logits(h_, x_, y_, n, per_, loss_, total, value, s), "tts_loss_bce_logits")

    for bad in (dict(h_=None), dict(x_=None), dict(y_=None), dict(per_=None), dict(loss_=None), dict(total=None),
                dict(count=None), dict(value=None)):
        with pytest.raises(RuntimeError, match="null"):
            masked(**bad)
    for bad in (dict(B_=0), dict(T_=0), dict(D_=-1)):
        with pytest.raises(RuntimeError, match="positive"):
            masked(**bad)
    for bad in (dict(xp=T * D - 1), dict(yp=T * D - 1)):
        with pytest.raises(RuntimeError, match="pitch"):
            masked(**bad)
    with pytest.raises(RuntimeError, match="negative"):
        masked(lens=(3, -1))
    with pytest.raises(RuntimeError, match="kind"):
        masked(kind=2)
    for bad in (dict(h_=None), dict(x_=None), dict(y_=None), dict(per_=None), dict(loss_=None), dict(total=None),
                dict(value=None)):
        with pytest.raises(RuntimeError, match="null"):
            bce(**bad)
    with pytest.raises(RuntimeError, match="positive"):
        bce(n=0)
    torch.cuda.synchronize()
    assert bool((per == 7.0).all()) and float(loss) == 7.0  # nothing was launched
    assert [v.value for v in host.values()] == [7.0, 7, 7.0]
    masked()  # the same arguments, valid
    assert per.tolist() == [15.0, 15.0] and float(loss) == 1.0
    assert [v.value for v in host.values()] == [30.0, 30, 1.0]
    masked(lens=None)
    assert host["count"].value == 30
    bce()
    assert host["value"].value == pytest.approx(1.3132616875182228, rel=1e-15)  # 1 + log1p(exp(-1))
    lib.tts_loss_destroy(h)
