"""CPU: the comparator of the encoder contract tests (encoder_util.assert_encoder_close) rejects the
mistakes the encoder kernels can make.  Each mistake is made in the fp64 oracle at L = 17 (one frame
past a 16-frame tile), its size is measured here, and the mutated result is handed to the
comparator as ``got``.  The reference helper itself is pinned to the reference's fixtures."""
import numpy as np
import pytest

import encoder_util as eu
from conftest import golden, golden_flags, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle

L = 17


@pytest.fixture(scope="module")
def base():
    """One sentence, zero state: ids, reference out [1, L, 512] and state [4, 1, 256]."""
    ids = eu.sentence(L)
    out, st = eu.ref_encoder_batch(eu.oracle(), [ids])
    return ids, out, st


def _mutant(edit):
    """The fp64 oracle on weights changed by ``edit(sd)``."""
    sd = {k: np.array(v) for k, v in weights_mod().tacotron2_weights(0).items()}
    edit(sd)
    return Tacotron2Oracle(sd, dtype=np.float64, **golden_flags(golden("t2_fwdmask_L100")))


def _rejected(got, ref, lens, got_state=None, ref_state=None):
    with pytest.raises(AssertionError):
        eu.assert_encoder_close(got, ref, lens, got_state, ref_state)


def test_bounds_are_the_projects():
    import test_gpu_parity as p
    assert eu.MEL_RTOL == p.MEL_RTOL and eu.ALIGN_ATOL == p.ALIGN_ATOL


def test_correct_results_pass(base):
    """The reference rounded to fp32 and the fp32 oracle (a correct fp32 implementation) pass, with
    and without a caller state; an Lmax above the sentence passes with zero rows."""
    ids, ref, st = base
    eu.assert_encoder_close(ref.astype(np.float32), ref, [L], st.astype(np.float32), st)
    o32, s32 = eu.ref_encoder_batch(eu.oracle(np.float32), [ids])
    e = eu.assert_encoder_close(o32, ref, [L], s32, st)
    print("fp32 oracle vs fp64 oracle, zero state:", {k: max(v) for k, v in e.items()})
    state = eu.split_state(eu.draw_state(1, 7))
    ref2, st2 = eu.ref_encoder_batch(eu.oracle(), [ids], state)
    o32, s32 = eu.ref_encoder_batch(eu.oracle(np.float32), [ids], state)
    e = eu.assert_encoder_close(o32, ref2, [L], s32, st2)
    print("fp32 oracle vs fp64 oracle, caller state:", {k: max(v) for k, v in e.items()})
    assert rel_rms(ref2, ref) > 1e-3  # (the state matters)
    pad = np.concatenate([ref, np.zeros((1, 3, 512))], axis=1)
    eu.assert_encoder_close(pad.astype(np.float32), pad, [L])


@pytest.mark.parametrize("sfx,half", [("", 0), ("_reverse", 1)])
def test_swapped_gate_rows_are_rejected(base, sfx, half):
    """W_hh rows of unit 10's input and forget gates exchanged, in one direction."""
    ids, ref, st = base

    def edit(sd):
        w = sd["encoder.lstm.weight_hh_l0" + sfx]
        w[[10, 256 + 10]] = w[[256 + 10, 10]]

    got, gst = eu.ref_encoder_batch(_mutant(edit), [ids])
    sl = slice(256 * half, 256 * half + 256)
    size = rel_rms(got[0, :, sl], ref[0, :, sl])
    print(f"swapped gate rows{sfx}: rel RMS {size:.2e} on that direction")
    other = slice(256 * (1 - half), 256 * (1 - half) + 256)
    assert size > eu.MEL_RTOL and np.array_equal(got[0, :, other], ref[0, :, other])
    _rejected(got, ref, [L])
    _rejected(ref, ref, [L], gst, st)  # ... and by the state alone


def test_zeroed_recurrence_is_rejected(base):
    ids, ref, st = base

    def edit(sd):
        sd["encoder.lstm.weight_hh_l0"][:] = 0
        sd["encoder.lstm.weight_hh_l0_reverse"][:] = 0

    got, _ = eu.ref_encoder_batch(_mutant(edit), [ids])
    print(f"W_hh zeroed: rel RMS {rel_rms(got, ref):.2e}")
    # step 0 of each direction has h = 0 either way
    assert np.array_equal(got[0, 0, :256], ref[0, 0, :256]) and np.array_equal(got[0, -1, 256:], ref[0, -1, 256:])
    _rejected(got, ref, [L])


def test_frames_past_the_length_leaking_in_are_rejected(base):
    """Six foreign frames past L (a convolution reading its halo from the next sentence or from
    padding ids): the forward half alone, which never runs over them, already differs."""
    ids, ref, _ = base
    longer = np.concatenate([ids, eu.sentence(6, 3)])
    got = eu.ref_encoder_batch(eu.oracle(), [longer])[0][:, :L]
    fwd = rel_rms(got[0, :, :256], ref[0, :, :256])
    print(f"halo leak: rel RMS {fwd:.2e} forward half, {rel_rms(got, ref):.2e} whole")
    assert fwd > eu.MEL_RTOL
    _rejected(got, ref, [L])
    fwd_only = ref.copy()
    fwd_only[0, :, :256] = got[0, :, :256]
    _rejected(fwd_only, ref, [L])


def test_exchanged_sentences_are_rejected():
    """Two sentences of one length exchanged (a wrong sentence-group offset), outputs or states."""
    ids_list = [eu.sentence(L, 0), eu.sentence(5), eu.sentence(L, 1)]
    ref, st = eu.ref_encoder_batch(eu.oracle(), ids_list)
    lens = [L, 5, L]
    eu.assert_encoder_close(ref, ref, lens, st, st)
    _rejected(ref[[2, 1, 0]], ref, lens)
    _rejected(ref, ref, lens, st[:, [2, 1, 0]], st)


def test_nonzero_row_past_the_length_is_rejected():
    ids_list = [eu.sentence(L), eu.sentence(5)]
    ref, _ = eu.ref_encoder_batch(eu.oracle(), ids_list)
    for bad in (1e-30, -0.5, np.nan):
        got = ref.copy()
        got[1, 5, 300] = bad
        _rejected(got, ref, [L, 5])
    got = ref.copy()
    got[1, L - 1, 0] = 1e-30  # the last padding row
    _rejected(got, ref, [L, 5])


def test_zero_final_state_is_rejected(base):
    """h_n = c_n = 0 with a correct output: what a path that never stores its final state returns."""
    _, ref, st = base
    for rows in (slice(0, 2), slice(2, 4), slice(0, 4), slice(1, 2)):
        got = st.copy()
        got[rows] = 0
        _rejected(ref, ref, [L], got, st)
    with pytest.raises(AssertionError):
        eu.assert_encoder_close(ref, ref, [L], None, st)


def test_batches_hold_what_the_gpu_cases_need():
    for B in (2, 3, 4, 5, 16, 17, 61, 64):
        lens = eu.group_lens(B)
        assert len(lens) == B and min(lens) == 1 and max(lens) <= 24 and lens[0] < max(lens)
        assert len(set(lens)) == min(B, 24)
        if B >= 16:  # a sentence of length <= 2 in the group of the (first) longest one
            G = (B + 3) // 4
            g = lens.index(max(lens)) // G
            assert min(lens[g * G:g * G + G]) <= 2
        ids = eu.sentences(lens)
        assert [len(x) for x in ids] == lens
        assert len({x.tobytes() for x in ids}) == B  # no two sentences share ids
    assert max(eu.group_lens(64)) == 24
    for Lmax, edges in ((17, [16, 17, 17]), (65, [16, 17, 32, 33, 64, 65]), (66, [16, 17, 32, 33, 64, 66])):
        lens = eu.dispatch_lens(Lmax)
        assert len(lens) == 64 and max(lens) == Lmax and lens[0] != Lmax and min(lens) >= 1
        assert sorted(x for x in lens if x > 12) == edges
        assert len({x.tobytes() for x in eu.sentences(lens)}) == 64
    # the frames that choose the convolution kernel (conv1d.hip launch_kw)
    assert 64 * 17 > 1024 and 64 * 17 <= 4096 and 64 * 65 > 4096 and 64 * 24 > 1024


def test_reference_matches_the_fixture():
    z = golden("t2_fwdmask_L12")
    out, _ = eu.ref_encoder_batch(eu.oracle(), [z["ids"]])
    assert out.shape == (1, 12, 512)
    assert rel_rms(out[0], z["enc"]) < eu.MEL_RTOL


def test_reference_threads_the_state_like_inference_truncated():
    z = golden("trunc_t2_3texts")
    texts = [z[f"ids{i}"] for i in range(3)]
    orc = Tacotron2Oracle(weights_mod().tacotron2_weights(0), dtype=np.float64, **golden_flags(z))
    want = orc.inference_truncated(texts)
    state = None
    for i, ids in enumerate(texts):
        out, st = eu.ref_encoder_batch(eu.oracle(), [ids], None if state is None else [state])
        assert rel_rms(out[0], want[i]["enc"]) < 1e-12, i
        state = eu.split_state(st)[0]
    alone, _ = eu.ref_encoder_batch(eu.oracle(), [texts[1]])
    assert rel_rms(alone[0], want[1]["enc"]) > 1e-3  # (the carry matters)


def test_reference_layout_and_cache():
    """Padded rows are zero, the state is [h_fwd, h_bwd, c_fwd, c_bwd] x [B], a cached sentence is
    returned unchanged, and a caller state keys the cache."""
    ids_list = [eu.sentence(3), eu.sentence(L)]
    out, st = eu.ref_encoder_batch(eu.oracle(), ids_list)
    assert out.shape == (2, L, 512) and st.shape == (4, 2, 256)
    assert np.all(out[0, 3:] == 0)
    # h_n: the forward direction ends at the last frame, the backward one at the first
    assert np.array_equal(st[0, 0], out[0, 2, :256]) and np.array_equal(st[1, 0], out[0, 0, 256:])
    assert np.array_equal(st[0, 1], out[1, L - 1, :256]) and np.array_equal(st[1, 1], out[1, 0, 256:])
    out[:] = 7.0  # the caller's copy is its own
    again, st2 = eu.ref_encoder_batch(eu.oracle(), ids_list)
    assert np.array_equal(st, st2) and np.abs(again).max() < 1.0
    with_state, _ = eu.ref_encoder_batch(eu.oracle(), ids_list, eu.split_state(eu.draw_state(2, 1)))
    assert rel_rms(with_state, again) > 1e-3
