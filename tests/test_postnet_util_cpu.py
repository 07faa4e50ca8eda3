"""CPU: the comparator of the Postnet / PostCBHG contract tests (postnet_util.assert_postnet_close)
rejects the mistakes the convolution kernels behind them can make.  Each mistake is made in the
fp64 oracle at T = 17 (one frame past a 16-frame tile), its size is measured and printed here, and
the mutated result is handed to the comparator as ``got``, shaped as the device call returns it.
The reference helpers are pinned to the reference's fixtures, and the case lists are checked for
the sums and products that choose the kernel (csrc/conv1d.hip launch_kw / launch_small)."""
import numpy as np
import pytest

import postnet_util as pu
from conftest import golden, golden_flags, rel_rms, weights_mod
from oracle.tacotron_oracle import TacotronOracle, _sig
from postnet_util import GST, T2

T = 17
FOREIGN = pu.mel(6, 9)  # frames of another sentence


def _got(which, arr, Tmax=None):
    return pu.pad_out(which, [arr], Tmax)


def _rejected(which, got, mels, refs, match=None):
    with pytest.raises(AssertionError, match=match):
        pu.assert_postnet_close(which, got, mels, refs)


def _gst_mutant(edit=None, cls=TacotronOracle, **kw):
    sd = {k: np.array(v) for k, v in weights_mod().tacotron_gst_weights(0).items()}
    if edit:
        edit(sd)
    return cls(sd, **dict(golden_flags(golden("gst_L10_nostyle")), dtype=np.float64), **kw)


def test_bounds_are_the_projects():
    import test_gpu_parity as p
    assert pu.MEL_RTOL is p.MEL_RTOL and pu.ALIGN_ATOL is p.ALIGN_ATOL
    assert pu.MEL_RTOL == 4e-6 and pu.ALIGN_ATOL == 4e-6


@pytest.mark.parametrize("which", [T2, GST])
def test_correct_results_pass(which):
    """The fp64 reference rounded to fp32 and the fp32 oracle (a correct fp32 implementation) pass,
    at lengths below the halo, on tile edges and with Tmax above the sentence."""
    for Tn in (1, 2, 5, 16, T, 33):
        m, r = pu.mel(Tn), pu.ref(which, Tn)
        pu.assert_postnet_close(which, _got(which, r), [m], [r])
        e = pu.assert_postnet_close(which, _got(which, pu.ref(which, Tn, dtype=np.float32), Tn + 7), [m], [r])
        print(f"{which} fp32 oracle vs fp64 oracle, T = {Tn}:", {k: max(v) for k, v in e.items()})
    sp = pu.specs([5, 0, T])
    refs = pu.ref_batch(which, sp)
    pu.assert_postnet_close(which, pu.pad_out(which, refs), [pu.mel(*s) for s in sp], refs)


def test_term_is_a_sixth_of_the_output():
    """U[0, 1) inputs: the postnet term's RMS against the output's (why the term has its own check)."""
    m, r = pu.mel(T).astype(np.float64), pu.ref(T2, T)
    term, out = float(np.sqrt(np.mean((r - m) ** 2))), float(np.sqrt(np.mean(r ** 2)))
    print(f"postnet term RMS {term:.3f}, output RMS {out:.3f}")
    assert 4 < out / term < 8


@pytest.mark.parametrize("which,n,floor", [(T2, 6, 1e-2), (GST, 6, 1e-3), (GST, 1, 3e-4), (T2, 1, 1e-3)])
def test_frames_past_the_length_leaking_in_are_rejected(which, n, floor):
    """n foreign frames past T (a kernel reading its halo, its pooling partner or its GRU input
    from rows past T_b, which in production hold an earlier, longer sentence)."""
    m, r = pu.mel(T), pu.ref(which, T)
    longer = np.concatenate([m, FOREIGN[:n]])
    got = np.asarray(pu.oracle(which).postnet(longer))[:T]
    size = rel_rms(got, r)
    print(f"{which}: {n} foreign frame(s) past T = {T}: rel RMS {size:.2e}")
    assert size > floor
    _rejected(which, _got(which, got), [m], [r])


def test_dropped_tile_halo_is_rejected():
    """The 16-frame tiles computed without their neighbours' rows (a halo dropped at t = 16): each
    tile as a sentence of its own.  The output hides it sixfold; the term does not."""
    m, r = pu.mel(T), pu.ref(T2, T)
    orc = pu.oracle(T2)
    got = np.concatenate([orc.postnet(m[:16]), orc.postnet(m[16:])])
    m64 = m.astype(np.float64)
    out, term = rel_rms(got, r), rel_rms(got - m64, r - m64)
    print(f"halo dropped at t = 16: out rel RMS {out:.2e}, term {term:.2e}")
    assert out > 1e-2 and term > 4 * out
    _rejected(T2, _got(T2, got), [m], [r])
    # one wrong row at the tile edge, right to 1e-5 everywhere else: the output check alone would
    # need the sixfold margin, the term check does not
    small = np.array(r)
    small[15:17] += 2e-5 * (got[15:17] - r[15:17])
    e = pu.postnet_errors(T2, _got(T2, small), [m], [r])
    print(f"  scaled to the bound: out {e['out_rel'][0]:.2e}, term {e['term_rel'][0]:.2e}")
    assert e["term_rel"][0] > 4 * e["out_rel"][0]


class _ShiftedBank8(TacotronOracle):
    """Bank member k = 8 padded [4, 3] instead of [3, 4]: its window one tap to the left."""

    def _bn_conv(self, prefix, x, k, pad_l, pad_r, act):
        if prefix.endswith("postnet.cbhg.conv1d_banks.7"):
            pad_l, pad_r = pad_r, pad_l
        return super()._bn_conv(prefix, x, k, pad_l, pad_r, act)


def test_shifted_even_bank_member_is_rejected():
    m, r = pu.mel(T), pu.ref(GST, T)
    got = _gst_mutant(cls=_ShiftedBank8).postnet(m)
    size = rel_rms(got, r)
    print(f"bank member k = 8 shifted one tap: rel RMS {size:.2e} ({size / pu.MEL_RTOL:.0f}x the bound)")
    assert size > 5 * pu.MEL_RTOL
    _rejected(GST, _got(GST, got), [m], [r])


class _PoolTail(TacotronOracle):
    """CBHG.forward with the max-pool's partner of the last frame taken from ``tail`` [K * 128]
    (what the bank buffer holds at row T_b) instead of the ConstantPad1d zero."""

    def __init__(self, *a, tail=None, **kw):
        super().__init__(*a, **kw)
        self.tail = tail

    def cbhg(self, prefix, x, K, projections):
        xt = x.T
        y = np.concatenate([self._bn_conv(f"{prefix}.conv1d_banks.{k - 1}", xt, k, (k - 1) // 2, k // 2, "relu")
                            for k in range(1, K + 1)], 0)
        yp = np.concatenate([y, self.tail[:, None]], 1)
        y = np.maximum(yp[:, :-1], yp[:, 1:])
        for i in range(len(projections)):
            y = self._bn_conv(f"{prefix}.conv1d_projections.{i}", y, 3, 1, 1, "relu" if i < len(projections) - 1 else None)
        y = y.T + x
        if projections[-1] != 128:
            y = y @ self.w[f"{prefix}.pre_highway.weight"].T
        for i in range(4):
            hp = f"{prefix}.highways.{i}"
            Hh = np.maximum(y @ self.w[hp + ".H.weight"].T + self.w[hp + ".H.bias"], 0)
            Tt = _sig(y @ self.w[hp + ".T.weight"].T + self.w[hp + ".T.bias"])
            y = Hh * Tt + y * (1.0 - Tt)
        return np.concatenate([self._gru_seq(f"{prefix}.gru", y, ""),
                               self._gru_seq(f"{prefix}.gru", y, "_reverse", reverse=True)], 1)


def test_pool_without_its_zero_is_rejected():
    """pool2 reading row T_b of the bank buffer (a longer sentence's bank output) instead of zero."""
    m, r = pu.mel(T), pu.ref(GST, T)
    same = _gst_mutant(cls=_PoolTail, tail=np.zeros(8 * 128)).postnet(m)
    assert rel_rms(same, r) < 1e-14  # (the restated forward is the oracle's)
    o = pu.oracle(GST)
    longer = np.concatenate([m, FOREIGN[:4]]).astype(np.float64).T
    tail = np.concatenate([o._bn_conv(f"postnet.cbhg.conv1d_banks.{k - 1}", longer, k, (k - 1) // 2, k // 2, "relu")
                           for k in range(1, 9)], 0)[:, T]
    got = _gst_mutant(cls=_PoolTail, tail=tail).postnet(m)
    size = rel_rms(got, r)
    print(f"pool2 without the zero at T_b: rel RMS {size:.2e} ({size / pu.MEL_RTOL:.0f}x the bound)")
    assert size > 5 * pu.MEL_RTOL
    _rejected(GST, _got(GST, got), [m], [r])


def test_exchanged_highway_columns_are_rejected():
    m, r = pu.mel(T), pu.ref(GST, T)

    def edit(sd):
        for n in ("weight", "bias"):
            h, t = "postnet.cbhg.highways.2.H." + n, "postnet.cbhg.highways.2.T." + n
            sd[h], sd[t] = sd[t], sd[h]

    got = _gst_mutant(edit).postnet(m)
    print(f"Highway layer 2 H / T exchanged: rel RMS {rel_rms(got, r):.2e}")
    _rejected(GST, _got(GST, got), [m], [r])


def test_exchanged_gru_directions_are_rejected():
    m, r = pu.mel(T), pu.ref(GST, T)

    def edit(sd):
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            f, b = f"postnet.cbhg.gru.{n}_l0", f"postnet.cbhg.gru.{n}_l0_reverse"
            sd[f], sd[b] = sd[b], sd[f]

    got = _gst_mutant(edit).postnet(m)
    print(f"GRU directions exchanged: rel RMS {rel_rms(got, r):.2e}")
    _rejected(GST, _got(GST, got), [m], [r])


@pytest.mark.parametrize("which", [T2, GST])
def test_exchanged_sentences_are_rejected(which):
    """Two sentences of one length exchanged (a wrong batch offset)."""
    sp = pu.specs([T, 5, T])
    mels, refs = [pu.mel(*s) for s in sp], pu.ref_batch(which, sp)
    pu.assert_postnet_close(which, pu.pad_out(which, refs), mels, refs)
    _rejected(which, pu.pad_out(which, [refs[2], refs[1], refs[0]]), mels, refs)


@pytest.mark.parametrize("which", [T2, GST])
def test_written_row_past_the_length_is_rejected(which):
    sp = pu.specs([T, 5, 0])
    mels, refs = [pu.mel(*s) for s in sp], pu.ref_batch(which, sp)
    good = pu.pad_out(which, refs, T + 3)
    pu.assert_postnet_close(which, good, mels, refs)
    for b, t, c in ((1, 5, 40), (1, T + 2, 0), (0, T, 79), (2, 0, 3)):
        for bad in (1e-30, 0.5, np.nan) + ((0.0,) if which == T2 else ()):
            got = good.copy()
            got[b, t, c] = bad
            _rejected(which, got, mels, refs, match="past T")
    if which == T2:  # zero-filled padding is a write too: the caller's rows are not the call's to touch
        _rejected(which, pu.pad_out(which, refs, T + 3, fill=0.0), mels, refs, match="past T")


@pytest.mark.parametrize("which", [T2, GST])
def test_nan_in_a_valid_row_is_reported(which):
    m, r = pu.mel(T), pu.ref(which, T)
    got = _got(which, r)
    got[0, 16, 7] = np.nan
    _rejected(which, got, [m], [r], match="1 NaN in valid rows")


def test_reference_matches_the_fixtures():
    z = golden("t2_fwdmask_L12")
    assert rel_rms(pu.oracle(T2).postnet(z["mel"]), z["mel_post"]) < pu.MEL_RTOL
    z = golden("gst_L10_nostyle")
    assert rel_rms(pu.oracle(GST).postnet(z["mel"]), z["linear"]) < pu.MEL_RTOL


def test_reference_cache_and_inputs():
    a, b = pu.mel(T, 0), pu.mel(T, 1)
    assert a.shape == (T, 80) and a.dtype == np.float32 and 0 <= a.min() and a.max() < 1
    assert not np.array_equal(a, b) and pu.mel(T, 0) is a and not a.flags.writeable
    r = pu.ref(T2, T)
    assert pu.ref(T2, T) is r and not r.flags.writeable and r.shape == (T, 80) and r.dtype == np.float64
    assert pu.ref(GST, T).shape == (T, 1025) and pu.ref(GST, 0).shape == (0, 1025)
    assert pu.specs([5, 17, 5, 5]) == [(5, 0), (17, 0), (5, 1), (5, 2)]
    pad = pu.pad_out(T2, [r[:3]], 5)
    assert np.all(pad[0, 3:].view(np.uint32) == pu.SENTINEL_BITS) and np.isnan(pad[0, 3:]).all()
    assert np.all(pu.pad_out(GST, [pu.ref(GST, 2)], 4)[0, 2:] == 0)


def test_batches_hold_what_the_gpu_cases_need():
    """The sums and products by which launch_kw / launch_small choose the kernel (small limit 1024
    frames, 16-channel tiles while the 32-channel grid is <= 128 workgroups, split-K below 256
    16-frame output tiles, 16-frame tiles to 4096 frames, varlen / 32- / 64-frame tiles above)."""
    def small_grid(B, Tlong, co_pad):  # the 32-channel grid of launch_small
        return B * -(-Tlong // 16) * (co_pad // 32)

    def tiles16(B, Tlong, co_pad):  # launch_kw's 16-frame output tiles
        return B * -(-Tlong // 16) * (co_pad // 64)

    # a: 16-channel tap kernel on layers 1-4 up to T = 128
    assert small_grid(1, 128, 512) <= 128 and small_grid(1, 128, 128) <= 128
    # b: T = 129 -> 32-channel on layers 1-3, 16-channel on layer 4; [5, 180, 33] -> 32 everywhere
    assert small_grid(1, 129, 512) > 128 and small_grid(1, 129, 128) <= 128 and 129 <= 1024
    assert small_grid(3, 180, 128) > 128 and 5 + 180 + 33 <= 1024
    # c: T = 1025 -> past the small limit; layers 0-3 have >= 256 tiles, layer 4 splits four ways
    assert 1025 > 1024 and tiles16(1, 1025, 512) >= 256 and tiles16(1, 1025, 128) == 130
    assert 130 * 4 <= 1024 < 130 * 8 and (512 // 16) % 4 == 0 and 4 * 1028 * 128 <= 1 << 20
    # d
    d = pu.lens_tiled16()
    assert len(d) == 64 and min(d) == 16 and max(d) == 33 and d[0] != 33 and 1024 < sum(d) <= 4096
    assert {16, 17, 32, 33} <= set(d) and tiles16(64, 33, 128) >= 256
    # e
    e = pu.lens_varlen()
    assert len(e) == 64 and sum(e) == 4100 and {63, 64, 65} <= set(e) and 58 <= min(e) and max(e) <= 70
    assert e[0] != max(e) and tiles16(64, max(e), 128) >= 256
    # PostCBHG above 4096 frames
    g = pu.lens_cbhg64()
    assert len(g) == 32 and sum(g) == 4100 and {63, 64, 65, 129} <= set(g) and max(g) <= 142 and g[0] != max(g)
    for lens in (d, e, g):
        sp = pu.specs(lens)
        assert len(set(sp)) == len(lens) and len({pu.mel(*s).tobytes() for s in sp}) == len(lens)
