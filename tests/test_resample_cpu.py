"""CPU: the host half of load_wav(sr=...) (audio.resample_filter, audio.resample_lengths) and the numpy
comparator the device resampler is held to (resample_util): its two restatements agree bitwise, and it tells
apart the two deviations a kernel is most likely to make (a multiplied time register, a float64 accumulator)."""
import numpy as np
import pytest

import resample_util as ru
from conftest import load_pkg


def test_kaiser_best_filter():
    audio = load_pkg("audio")
    half_win, num_table = audio.resample_filter()
    assert num_table == 512 and half_win.shape == (32769,) and half_win.dtype == np.float64
    assert half_win[0] == 0.9475937167399596
    # (computed with scipy 1.15.3; the margin covers i0 and summation differences of a few ulp)
    assert half_win[512] == pytest.approx(0.05207910617885589, rel=1e-12)
    assert half_win[-1] == pytest.approx(1.6401183069347287e-08, rel=1e-12)
    assert half_win.sum() == pytest.approx(256.4737964902581, rel=1e-12)
    assert np.array_equal(half_win, audio.resample_filter("kaiser_best")[0])
    assert np.array_equal(half_win, ru.kaiser_best()[0]) and ru.kaiser_best()[1] == 512
    with pytest.raises(NotImplementedError):
        audio.resample_filter("kaiser_fast")
    small, table = ru.small_filter()
    assert small.shape == (33,) and table == 8


@pytest.mark.parametrize("args,want", [((3000, 48000, 22050), (1378, 1379)), ((3001, 44100, 22050), (1500, 1501)),
                                       ((2205, 22050, 16000), (1600, 1600)), ((1280, 32000, 22050), (882, 882)),
                                       ((3, 48000, 22050), (1, 2))])
def test_resample_lengths(args, want):
    audio = load_pkg("audio")
    assert audio.resample_lengths(*args) == want
    assert ru.lengths(*args) == want


def test_resample_lengths_refuses_an_empty_result():
    with pytest.raises(ValueError):
        load_pkg("audio").resample_lengths(2, 48000, 22050)


@pytest.mark.parametrize("orig,target,N", [(48000, 22050, 50), (16000, 22050, 40)])
def test_comparator_restatements_agree(orig, target, N):
    x = ru.signal(N, orig)
    a, b = ru.resample_ref(x, orig, target), ru.resample_literal(x, orig, target)
    assert a.dtype == b.dtype == np.float32 and len(a) == ru.lengths(N, orig, target)[1]
    assert np.array_equal(ru.bits(a), ru.bits(b))
    assert np.abs(a).max() > 0.1


def test_comparator_has_teeth():
    orig, target, N = 48000, 22050, 3000
    x = ru.signal(N, orig)
    n_res = ru.lengths(N, orig, target)[0]
    inc = 1.0 / (float(target) / orig)
    serial, product = ru.time_register(n_res, inc), ru.time_register(n_res, inc, serial=False)
    flips = int((serial.astype(np.int64) != product.astype(np.int64)).sum())
    ref = ru.bits(ru.resample_ref(x, orig, target))[:n_res]
    by_product = ru.bits(ru.resample_ref(x, orig, target, serial_register=False))[:n_res]
    by_f64 = ru.bits(ru.resample_ref(x, orig, target, acc_dtype=np.float64))[:n_res]
    print("register flips", flips, "samples changed by t * inc", int((ref != by_product).sum()),
          "by a float64 accumulator", int((ref != by_f64).sum()), "of", n_res)
    assert (ref != by_product).sum() >= 1
    assert (ref != by_f64).sum() > n_res // 2
    # the pass-through is the input itself
    assert np.array_equal(ru.resample_ref(x, orig, orig), x)
