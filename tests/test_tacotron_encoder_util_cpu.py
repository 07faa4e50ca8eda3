"""CPU: the helpers of the Tacotron / TacotronGST encoder contract tests (tacotron_encoder_util.py)
checked without a GPU: the case lists, the sharpened weights, the mutants' arithmetic, the
constants the bounds are built from (re-measured from the two oracles), the sensitivity condition
(every mutant moves its term by at least 10x the term's bound at every GPU shape where it is not the
identity), the reason the sharpened model exists (the shipped weights hide another sentence's
style under the project's bound), and the comparator on outputs that must pass and must fail."""
import numpy as np
import pytest

import tacotron_encoder_util as u
from conftest import golden, rel_rms
from tacotron_encoder_util import GSTM, SHARP, TACO


# ---------------------------------------------------------------------------- case lists, weights
def test_lens_tiled64():
    a, b, c = (u.lens_tiled64(t) for t in (4096, 4097, 4098))
    assert (sum(a), sum(b), sum(c)) == (4096, 4097, 4098) and len(a) == len(b) == len(c) == 64
    assert a[:63] == b[:63] == c[:63] and (a[63], b[63], c[63]) == (64, 65, 66)
    assert set(a) == set(u.LENS_64)
    assert a[0] != max(a)  # the longest sentence is not the first
    assert len(set(u.specs(a, 2))) == 16
    assert u.expect_kinds(sum(a), False) == [u.KIND_TILED16] * 10 + [-1]
    assert u.expect_kinds(sum(b), True) == [u.KIND_TILED64] * 10 + [u.KIND_TILED16]


def test_h6_steps():
    assert [u.h6_of(t) for t in u.STYLE_TS] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 4]


def test_sharpen_touches_gst_entries_only():
    base = u.weights_mod().tacotron_gst_weights(0)
    sharp = u.state_dict(SHARP)
    changed = [k for k in base if not np.array_equal(base[k], sharp[k])]
    assert sorted(changed) == sorted(k for k, _ in u.SHARPEN) and all(k.startswith("gst.") for k in changed)
    for k, f in u.SHARPEN:
        assert np.array_equal(sharp[k], base[k] * np.float32(f))
    # the three models share every encoder tensor, so one encoder reference serves GSTM and SHARP
    for k, v in u.state_dict(GSTM).items():
        if k.startswith(("embedding", "encoder.")):
            assert np.array_equal(v, sharp[k]) and np.array_equal(v, u.state_dict(TACO)[k]), k
    assert "speaker_embedding.weight" not in u.state_dict(TACO) and not any(k.startswith("gst.") for k in u.state_dict(TACO))


def test_shipped_oracle_is_the_goldens():
    """The helper's oracle on the shipped weights reproduces the reference's fixture (encoder output
    with speaker and style, and the GST vector)."""
    z = golden("gst_L24_style_spk")
    o = u.oracle(GSTM)
    assert rel_rms(o.gst(z["style_mel"]), z["gst"]) < 1e-6
    assert rel_rms(o.encoder(z["ids"], int(z["speaker_id"]), z["style_mel"]), z["enc"]) < 1e-6


# ---------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("L", [1, 9, 33])
def test_cbhg_mutant_none_is_the_oracle(L):
    o = u.oracle(GSTM)
    assert np.array_equal(u.encoder_mutant(GSTM, L, 0), o.encoder(u.ids_of(L, 0)))
    assert np.array_equal(u.encoder_mutant(GSTM, L, 0), u.enc_ref(GSTM, L, 0))


@pytest.mark.parametrize("Ts", [1, 65, 200])
def test_gst_mutant_none_is_the_oracle(Ts):
    for which in (GSTM, SHARP):
        assert np.array_equal(u.gst_mutant(u.oracle(which), u.style_of(Ts)), u.oracle(which).gst(u.style_of(Ts)))


def _cbhg_shapes():
    """(L, k, Lmax) of every sentence of a GPU encoder case on the GST model."""
    s = {(L, 0, L) for L in u.LENS_B1}
    for lens, Lmax in u.RAGGED:
        s |= {(L, k, Lmax) for L, k in u.specs(lens)}
    for total in (4096, 4097, 4098):
        lens = u.lens_tiled64(total)
        s |= {(L, k, max(lens)) for L, k in u.specs(lens, 2)}
    return sorted(s)


def test_cbhg_mutants_reach_the_margin():
    """Every CBHG mutant moves the encoder term by >= 10x the project's relative-RMS bound (and so
    >= 44x the fp32-oracle bound) at every shape of the GPU cases, the listed identities apart."""
    seen = {m: 0 for m in u.CBHG_MUTANTS}
    for L, k, Lmax in _cbhg_shapes():
        ref = u.enc_ref(GSTM, L, k)
        for m in u.CBHG_MUTANTS:
            got = u.encoder_mutant(GSTM, L, k, m, Lmax)
            rel, _ = u.vec_errors(got, ref)
            if u.mutant_is_identity(m, L=L, Lmax=Lmax):
                assert rel == 0.0, (m, L, Lmax, rel)
                continue
            seen[m] += 1
            assert rel >= u.MARGIN * u.MEL_RTOL, f"{m} at L = {L}, Lmax = {Lmax}: moves the term by {rel:.2e} only"
    assert all(n >= 8 for n in seen.values()), seen


def _style_shapes():
    """(Ts, k, the next sentence's k or None) of every style a GPU case on the sharpened model
    compares with the oracle: batch-1 over STYLE_TS, the B = 5 and B = 64 batches at TS_BATCH."""
    s = [(Ts, 0, None) for Ts in u.STYLE_TS]
    s += [(u.TS_BATCH, b, (b + 1) % 5) for b in range(5)]
    s += [(u.TS_BATCH, b, (b + 1) % 64) for b in (0, 31, 63)]
    return s


def test_gst_mutants_reach_the_margin():
    """Every GST mutant moves the style term of the sharpened model by >= 10x the term's bound at
    every shape of the GPU cases, the listed identities apart (next_style: the batches only)."""
    o = u.oracle(SHARP)
    seen = {m: 0 for m in u.GST_MUTANTS}
    least = {}
    for Ts, k, nxt in _style_shapes():
        ref = u.gst_ref(SHARP, Ts, k)
        for m in u.GST_MUTANTS:
            if u.mutant_is_identity(m, Ts=Ts, B=1 if nxt is None else 5):
                if m not in ("drop_last_row", "next_style"):
                    assert np.array_equal(u.gst_mutant(o, u.style_of(Ts, k), m), ref), (m, Ts)
                continue
            got = u.gst_mutant(o, u.style_of(Ts, k), m, None if nxt is None else u.style_of(Ts, nxt))
            rel, _ = u.vec_errors(got, ref)
            seen[m] += 1
            least[m] = min(least.get(m, rel), rel)
            assert rel >= u.MARGIN * u.STYLE_REL[SHARP], f"{m} at Ts = {Ts}: moves the style term by {rel:.2e} only"
    print("smallest movement per GST mutant:", {m: f"{v:.2e}" for m, v in least.items()})
    assert seen["next_style"] == 8 and seen["hw_swap"] == 5 + 8 and seen["drop_last_row"] == len(u.STYLE_TS) - 1 + 8
    assert all(n >= 8 for n in seen.values()), seen


def test_shipped_weights_hide_the_style():
    """Why the sharpened model exists: on the shipped weights the next sentence's style moves the
    summed output of the B = 5 speaker batch by 1.1e-6 .. 1.8e-6, less than the project's 4e-6 bound,
    so no parity test of the sum sees it.  (Without a speaker the sum moves by 6e-6 .. 8.5e-6, about
    the bound, and the style term alone by 1.5e-5 .. 2.4e-5, 7 - 11x its own bound: short of the 10x
    margin asked of a mutant.)"""
    for b, ((L, k), s) in enumerate(zip(u.specs(u.LENS_B5), u.SPEAKERS)):
        enc = u.enc_ref(GSTM, L, k) + u.spk_row(s)[None, :]
        g, gn = u.gst_ref(GSTM, u.TS_BATCH, b), u.gst_ref(GSTM, u.TS_BATCH, (b + 1) % 5)
        moved = rel_rms(enc + gn[None, :], enc + g[None, :])
        assert 0 < moved < u.MEL_RTOL, (b, moved)
        # the same pair on the sharpened weights: three orders above the bound
        assert u.vec_errors(u.gst_ref(SHARP, u.TS_BATCH, (b + 1) % 5), u.gst_ref(SHARP, u.TS_BATCH, b))[0] > 1e-3


# ---------------------------------------------------------------------------- the constants
def _within(measured, const):
    """The constant is the figure measured when the helper was written, rounded up to two digits; the
    fp32 oracle's sums run in the BLAS of the machine, so a re-measurement may land a little to
    either side of it."""
    return const / 1.5 <= measured <= 1.25 * const


def test_fp32_constants_are_the_oracles_own():
    """ENC / SPK / STYLE constants: the fp32 oracle's worst against the fp64 oracle over the inputs
    of the GPU cases."""
    e = [u.f32_encoder(*x) for x in u.encoder_inputs()]
    assert _within(max(r for r, _ in e), u.ENC_F32_REL) and _within(max(a for _, a in e), u.ENC_F32_ABS), \
        (max(r for r, _ in e), max(a for _, a in e))
    s = [u.f32_speaker(L, k, sp) for (L, k), sp in zip(u.specs(u.LENS_B5), u.SPEAKERS)]
    assert _within(max(r for r, _ in s), u.SPK_F32_REL) and _within(max(a for _, a in s), u.SPK_F32_ABS), s
    for which in (SHARP, GSTM):
        s = [u.f32_style(which, *x) for x in u.style_inputs(which)]
        assert _within(max(r for r, _ in s), u.STYLE_F32_REL[which]), (which, max(r for r, _ in s))
        assert _within(max(a for _, a in s), u.STYLE_F32_ABS[which]), (which, max(a for _, a in s))
    assert u.ENC_REL < u.MEL_RTOL and u.ENC_ABS < u.ALIGN_ATOL  # the 10x rule is the tighter one


# ---------------------------------------------------------------------------- comparator
def _fp32_outputs(sp, Lmax, add=None):
    outs = []
    for b, (L, k) in enumerate(sp):
        h = u.enc_ref(GSTM, L, k, np.float32)
        outs.append(h if add is None else h + np.asarray(add[b], np.float32)[None, :])
    return u.pad_out(outs, Lmax)


def test_comparator_passes_the_fp32_oracle_and_fails_the_mutants():
    sp, Lmax = u.specs((9, 17)), 21
    lens = [L for L, _ in sp]
    refs = [u.enc_ref(GSTM, L, k) for L, k in sp]
    none = _fp32_outputs(sp, Lmax)
    u.assert_encoder_term(none, lens, refs)
    for m in u.CBHG_MUTANTS:
        bad = u.pad_out([u.encoder_mutant(GSTM, L, k, m, Lmax).astype(np.float32) for L, k in sp], Lmax)
        with pytest.raises(AssertionError, match="rel RMS"):
            u.assert_encoder_term(bad, lens, refs)
    # a 1e-6 relative error hides under the project's bound but not under the fp32-oracle rule
    with pytest.raises(AssertionError, match="above 10x the fp32 oracle"):
        u.assert_encoder_term((none * np.float32(1 + 1.5e-6)).astype(np.float32), lens, refs)
    # rows past L: -0.0, NaN and the sentinel all fail
    for poison in (np.float32(-0.0), np.float32("nan")):
        bad = none.copy()
        bad[0, 9, 5] = poison
        with pytest.raises(AssertionError, match="past L"):
            u.assert_encoder_term(bad, lens, refs)
    bad = none.copy()
    bad.view(np.uint32)[1, 20, 255] = u.SENTINEL_BITS
    with pytest.raises(AssertionError, match="past L"):
        u.assert_encoder_term(bad, lens, refs)
    bad = none.copy()
    bad[1, 3, 7] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        u.assert_encoder_term(bad, lens, refs)
    # speaker term
    rows = [u.spk_row(s) for s in (3, 0)]
    spk = _fp32_outputs(sp, Lmax, rows)
    u.assert_added_term(spk, none, lens, rows, u.SPK_REL, u.SPK_ABS, "speaker term")
    with pytest.raises(AssertionError, match="speaker term"):
        u.assert_added_term(spk, none, lens, rows[::-1], u.SPK_REL, u.SPK_ABS, "speaker term")
    # style term on the sharpened weights: the fp32 oracle passes, every mutant fails
    o = u.oracle(SHARP)
    g32 = [u.gst_ref(SHARP, u.TS_BATCH, b, np.float32) for b in range(2)]
    g64 = [u.gst_ref(SHARP, u.TS_BATCH, b) for b in range(2)]
    u.assert_added_term(_fp32_outputs(sp, Lmax, g32), none, lens, g64, u.STYLE_REL[SHARP], u.STYLE_ABS[SHARP], "style term")
    for m in u.GST_MUTANTS:
        gm = [u.gst_mutant(o, u.style_of(u.TS_BATCH, b), m, u.style_of(u.TS_BATCH, 1 - b)) for b in range(2)]
        with pytest.raises(AssertionError, match="style term"):
            u.assert_added_term(_fp32_outputs(sp, Lmax, gm), none, lens, g64, u.STYLE_REL[SHARP], u.STYLE_ABS[SHARP],
                                "style term")


def test_padded_ids_are_no_table_rows():
    ids, lens, Lmax = u.padded_ids(u.specs((4, 33, 1, 16)), 40)
    assert ids.dtype == np.int32 and ids.shape == (4, 40) and lens == [4, 33, 1, 16] and Lmax == 40
    for b, L in enumerate(lens):
        assert ((ids[b, :L] >= 3) & (ids[b, :L] < 130)).all()
        assert set(ids[b, L:].tolist()) == {-1, 0x7FFFFFFF}
