"""GPU: the contracts of tts_postnet_run (csrc/postnet.hip) and tts_tacotron_postnet
(csrc/tacotron_api.hip run_cbhg + last_linear) on every convolution kernel the host can choose for
them (csrc/conv1d.hip launch_kw / launch_small), each call against the fp64 oracle sentence by
sentence (postnet_util.ref) under the project's bounds (postnet_util.assert_postnet_close: the
output and, for Tacotron2, the postnet term out - mel alone).  Input rows past T_b are NaN, the
output starts as a sentinel bit pattern: rows past T_b must come back as the sentinel
(tts_postnet_run) or exactly zero (tts_tacotron_postnet).  Every Tacotron2 case asserts the kernel
that served each of the five layers (tts_postnet_last_path, ConvKind of csrc/conv1d.h); another
kernel on a healthy MI355X is a failure.  One Tacotron2 model and one TacotronGST model serve
every case.

Measured on an MI355X (profiles/postnet_contract.json, worst sentence of any case): Postnet output
relative RMS <= 8.1e-8, postnet term <= 4.6e-7, max-abs <= 2.9e-7 on every kernel kind; PostCBHG
linear <= 4.6e-8 relative RMS, <= 7.6e-8 max-abs.  The fp32 oracle against the fp64 one gives
8.2e-8 / 4.7e-7 / 3.0e-7 and 4.9e-8 / 9.4e-8 on the same inputs.  Every case passed as the kernels
stood: the contract the header now states was already kept."""
import numpy as np
import pytest

import postnet_util as pu
from postnet_util import (GST, KIND_SMALL_CM, KIND_SMALL_TAP16, KIND_SMALL_TAP32, KIND_SPLITK_REDUCE, KIND_TILED16,
                          KIND_TILED32, KIND_VARLEN64, T2)

pytestmark = pytest.mark.gpu

SMALL16 = [KIND_SMALL_CM] + [KIND_SMALL_TAP16] * 4
SMALL32 = [KIND_SMALL_CM] + [KIND_SMALL_TAP32] * 4
SPLITK = [KIND_TILED16] * 4 + [KIND_SPLITK_REDUCE]


@pytest.fixture(scope="module")
def t2():
    return pu.make_model(max_batch=64)


@pytest.fixture(scope="module")
def gst():
    return pu.make_gst_model(max_batch=64)


# ============================================================================ Tacotron2 Postnet
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 128])
def test_postnet_batch1_lengths(t2, T):
    """a: lengths below the k = 5 halo and across the 16-frame tile edges; up to 128 frames the
    32-channel grid has <= 128 workgroups, so layers 1-4 take the 16-channel tap kernel."""
    pu.check_call(f"a_T{T}", T2, t2, pu.specs([T]), SMALL16)


@pytest.mark.parametrize("lens,kinds", [([129], [KIND_SMALL_CM] + [KIND_SMALL_TAP32] * 3 + [KIND_SMALL_TAP16]),
                                        ([5, 180, 33], SMALL32)])
def test_postnet_small_32_channel(t2, lens, kinds):
    """b: 9 frame tiles x 16 channel tiles = 144 workgroups on layers 1-3 (layer 4 has 4 channel
    tiles: 36); 36 frame tiles x 4 on layer 4 of the ragged batch."""
    pu.check_call("b_" + "_".join(map(str, lens)), T2, t2, pu.specs(lens), kinds)


def test_postnet_split_k(t2):
    """c: one 1025-frame sentence is past the small kernel's 1024 frames; layer 4 (Cin = 512,
    co_pad = 128) has 130 output tiles < 256 and splits its K steps four ways, summed by the
    reduce launch."""
    pu.check_call("c_T1025", T2, t2, pu.specs([1025]), SPLITK)


def test_postnet_tiled16_batch64(t2):
    """d: 64 sentences of 16..33 frames (1024 < sum <= 4096; 2 * 64 * 3 >= 256 tiles on layer 4)."""
    pu.check_call("d_B64_tiled16", T2, t2, pu.specs(pu.lens_tiled16()), [KIND_TILED16] * 5)


@pytest.mark.parametrize("vl", [None, 0])
def test_postnet_above_4096_frames(t2, vl):
    """e: 64 sentences, 4100 frames, lengths around the 64-frame tile: the variable-length tiles,
    and under TTS_CONV_VL=0 (read per launch) the 32-frame tiles; one set of references."""
    sp = pu.specs(pu.lens_varlen())
    if vl is None:
        pu.check_call("e_B64_varlen", T2, t2, sp, [KIND_VARLEN64] * 5)
    else:
        with pu._env(TTS_CONV_VL=vl):
            pu.check_call("e_B64_vl0", T2, t2, sp, [KIND_TILED32] * 5)


@pytest.mark.parametrize("lens,Tmax,kinds", [
    ([5, 0, 17], None, SMALL16), ([0], None, SMALL16), ([17], 24, SMALL16), ([5, 0, 17], 24, SMALL16),
    # 3 sentences x 3 frame tiles (of the longest, not of Tmax) x 16 channel tiles = 144 > 128 on layers 1-3
    ([3, 33, 16], 40, [KIND_SMALL_CM] + [KIND_SMALL_TAP32] * 3 + [KIND_SMALL_TAP16])])
def test_postnet_zero_lengths_and_tmax(t2, lens, Tmax, kinds):
    """f: T[b] = 0 is legal (that sentence is neither read nor written) and Tmax may exceed the
    longest sentence: the tail is NaN on the way in and the sentinel on the way out."""
    name = "f_" + "_".join(map(str, lens)) + (f"_Tmax{Tmax}" if Tmax else "")
    pu.check_call(name, T2, t2, pu.specs(lens), kinds, Tmax=Tmax)


def test_postnet_one_handle_many_shapes(t2):
    """g: shapes in turn on one handle.  The intermediate buffers keep the rows of the 1025-frame
    call; nothing of them shows in the shorter calls after it, and the repeated call is bitwise
    the first."""
    first = pu.check_call("g_1_T1025", T2, t2, pu.specs([1025]), SPLITK)
    pu.check_call("g_2_T3", T2, t2, pu.specs([3]), SMALL16)
    pu.check_call("g_3_5_0_17", T2, t2, pu.specs([5, 0, 17]), SMALL16, Tmax=24)
    pu.check_call("g_4_B64_varlen", T2, t2, pu.specs(pu.lens_varlen()), [KIND_VARLEN64] * 5)
    last = pu.check_call("g_5_T1025", T2, t2, pu.specs([1025]), SPLITK)
    assert first.shape == (1, 1025, 80) and np.array_equal(first, last)


# ============================================================================ PostCBHG
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 33])
def test_postcbhg_batch1_lengths(gst, T):
    """Lengths below the 8-tap bank window and the k = 3 projections' halo, and across the
    16-frame tile edges."""
    pu.check_call(f"cbhg_T{T}", GST, gst, pu.specs([T]))


@pytest.mark.parametrize("lens,Tmax", [([9, 17], 21), ([4, 33, 0, 16, 1], 40), ([0, 8], None)])
def test_postcbhg_ragged(gst, lens, Tmax):
    """Ragged batches with a T[b] = 0 sentence and Tmax above the longest: linear rows past T_b
    exactly zero, NaN input rows past T_b never read (bank halo, pool2 partner, GRU)."""
    pu.check_call("cbhg_" + "_".join(map(str, lens)), GST, gst, pu.specs(lens), Tmax=Tmax)


def test_postcbhg_above_4096_frames(gst):
    """32 sentences, 4100 frames: the 64-frame tiles of KW = 1 / 3 / 8, with 63, 64, 65 and 129
    frames among them."""
    pu.check_call("cbhg_B32_tiled64", GST, gst, pu.specs(pu.lens_cbhg64()))


def test_postcbhg_one_handle_many_shapes(gst):
    """The same handle through long, short, ragged and long again; the repeat is bitwise the first."""
    big = pu.specs(pu.lens_cbhg64())
    first = pu.check_call("cbhg_g_1_B32", GST, gst, big)
    pu.check_call("cbhg_g_2_T3", GST, gst, pu.specs([3]))
    pu.check_call("cbhg_g_3_ragged", GST, gst, pu.specs([4, 33, 0, 16, 1]), Tmax=40)
    pu.check_call("cbhg_g_4_T17", GST, gst, pu.specs([17]))
    last = pu.check_call("cbhg_g_5_B32", GST, gst, big)
    assert first.shape[0] == 32 and np.array_equal(first, last)
