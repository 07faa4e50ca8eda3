"""GPU: the Tacotron2 encoder's contract on every BiLSTM path and every convolution kernel the host
can choose (csrc/encoder_api.hip tts_encoder_run_state, csrc/conv1d.hip launch_kw / launch_small),
each call against the fp64 oracle run sentence by sentence (encoder_util.ref_encoder_batch) under
the project's bounds (encoder_util.assert_encoder_close).  Every case asserts the path that served
it (tts_encoder_last_path: 0 per-step launches, 1 resident batch-1, 2 batched resident); another
path on a healthy MI355X is a failure.  Two handles: one resident, one created under TTS_RESIDENT=0
whose every call takes the per-step launches.

Measured on an MI355X (profiles/encoder_contract.json, worst sentence of any case): relative RMS
<= 2.4e-7 on every path; max-abs of out / h_n <= 6.2e-8 and of c_n <= 9.9e-8.  The fp32 oracle
against the fp64 one gives 1.5e-7 / 7.8e-8 / 1.1e-7 on the same sentences."""
import numpy as np
import pytest

import encoder_util as eu
from encoder_util import PATH_PER_STEP, PATH_RESIDENT, PATH_RESIDENT_BATCH

pytestmark = pytest.mark.gpu

HANDLES = ["resident", "per_step"]


@pytest.fixture(scope="module")
def models():
    return {"resident": eu.make_model(64, resident=True), "per_step": eu.make_model(64, resident=False)}


def _path(handle, resident_path):
    return resident_path if handle == "resident" else PATH_PER_STEP


# ---------------------------------------------------------------------------- a, b: batch 1
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6, 15, 16, 17, 33])
def test_batch1_lengths(models, handle, L):
    """Lengths below the k = 5 halo and across the 16- and 32-frame tile edges, zero state."""
    eu.check_call(f"a_batch1_L{L}", handle, models[handle], [eu.sentence(L)], _path(handle, PATH_RESIDENT))


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("L,Lmax", [(5, 9), (16, 17)])
def test_batch1_padded(models, handle, L, Lmax):
    """lens[0] < Lmax: the per-step launches serve it on a resident handle too; rows past L are zero."""
    eu.check_call(f"b_batch1_L{L}_Lmax{Lmax}", handle, models[handle], [eu.sentence(L)], PATH_PER_STEP, Lmax=Lmax)


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("first_state", [False, True])
def test_batch1_state_chain(models, handle, first_state):
    """Three texts (4, 1 and 17 characters), each call's state_out the next call's state_in; the
    reference threads the oracle's own fp64 state."""
    m = models[handle]
    state = ref_state = eu.draw_state(1, 21) if first_state else None
    for i, L in enumerate((4, 1, 17)):
        _, state, ref_state = eu.check_call(f"c_chain{int(first_state)}_call{i}_L{L}", handle, m, [eu.sentence(L, 2)],
                                            _path(handle, PATH_RESIDENT), state_in=state, want_state=True,
                                            ref_state_in=ref_state)


# ---------------------------------------------------------------------------- d: sentence groups
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("B", [2, 3, 4, 5, 16, 17, 61, 64])
def test_batched_group_edges(models, handle, B):
    """Empty, partial and full sentence groups of the batched resident BiLSTM; every sentence
    against its own batch-1 reference."""
    eu.check_call(f"d_groups_B{B}", handle, models[handle], eu.sentences(eu.group_lens(B)),
                  _path(handle, PATH_RESIDENT_BATCH))


# ---------------------------------------------------------------------------- e: state, B >= 2
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("B", [3, 5])
def test_batched_state_in(models, handle, B):
    """A caller state routes the batch to the per-step launches on either handle."""
    eu.check_call(f"e_state_in_B{B}", handle, models[handle], eu.sentences(eu.group_lens(B)), PATH_PER_STEP,
                  state_in=eu.draw_state(B, 30 + B), want_state=True)


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("B", [2, 5, 64])
def test_batched_state_out_only(models, handle, B):
    """state_in = NULL, state_out set: the batched resident kernel stores (h_n, c_n) itself.
    Before it did, this call returned TTS_OK with h_n = c_n = 0 on the resident handle (all three
    batch sizes: 'sentence 0 (L = 1): h_n rel RMS 1.000e+00'); the per-step handle was right."""
    eu.check_call(f"e_state_out_B{B}", handle, models[handle], eu.sentences(eu.group_lens(B)),
                  _path(handle, PATH_RESIDENT_BATCH), want_state=True)


# ---------------------------------------------------------------------------- f: convolutions
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("Lmax,vl", [(17, None), (65, None), (66, 0)])
def test_conv_dispatch_at_batch64(models, handle, Lmax, vl):
    """B * Lmax frames choose the convolution kernel: 1088 -> conv_kernel<5,16,1,4>, 4160 ->
    conv_vl_kernel, 4224 under TTS_CONV_VL=0 -> conv_kernel<5,32,2,2> (the knob is read while the
    (B, Lmax) graph is captured, so that shape is used by this case alone)."""
    ids_list = eu.sentences(eu.dispatch_lens(Lmax))
    args = (f"f_conv_Lmax{Lmax}" + ("_vl0" if vl is not None else ""), handle, models[handle], ids_list,
            _path(handle, PATH_RESIDENT_BATCH))
    if vl is None:
        eu.check_call(*args)
    else:
        with eu._env(TTS_CONV_VL=vl):
            eu.check_call(*args)


# ---------------------------------------------------------------------------- g: one handle
@pytest.mark.parametrize("handle", HANDLES)
def test_one_handle_many_shapes(models, handle):
    """Shapes in turn on one handle: nothing of an earlier call (graphs, granules, h / c slots, the
    output buffer) shows in a later one; the repeated batch is bitwise the first.  (Rows past L_b
    on a replayed graph: a memset node there once left a stale 16-byte pattern in them after calls
    that copy a state out; a kernel zeroes them now.  test_batched_state_* replay the graphs of
    test_batched_group_edges and caught it.)"""
    m = models[handle]
    big = eu.sentences(eu.group_lens(64))
    first, _, _ = eu.check_call("g_shapes_1_B64", handle, m, big, _path(handle, PATH_RESIDENT_BATCH))
    eu.check_call("g_shapes_2_B2", handle, m, [eu.sentence(2, 1), eu.sentence(5, 1)], _path(handle, PATH_RESIDENT_BATCH),
                  want_state=True)
    eu.check_call("g_shapes_3_B1", handle, m, [eu.sentence(17, 1)], _path(handle, PATH_RESIDENT))
    eu.check_call("g_shapes_4_B1_padded", handle, m, [eu.sentence(5, 2)], PATH_PER_STEP, Lmax=9)
    last, _, _ = eu.check_call("g_shapes_5_B64", handle, m, big, _path(handle, PATH_RESIDENT_BATCH), want_state=True)
    assert first.shape == (64, 24, 512) and np.array_equal(first, last)


# ---------------------------------------------------------------------------- h: speakers
@pytest.fixture(scope="module")
def speaker_model():
    return eu.make_model(8, resident=True, num_speakers=6)


@pytest.mark.parametrize("lens,add_lens,spk", [([7], [7], [4]),
                                               ([9, 3, 17, 1, 6], [9, 3, 17, 0, 6], [5, 0, 5, 2, 1])])
def test_speaker_add(speaker_model, lens, add_lens, spk):
    """tts_encoder_add_speakers on the encoder's own output: the oracle's output plus the table row
    over t < lens[b]; a sentence passed with length 0 is left as it was, rows past L stay zero."""
    ids_list = eu.sentences(lens)
    ids, _ = eu.pad_ids(ids_list)
    enc, _, path = eu.run_encoder(speaker_model, ids, lens)
    assert path == (PATH_RESIDENT if len(lens) == 1 else PATH_RESIDENT_BATCH)
    got = eu.add_speakers(speaker_model, enc, add_lens, spk)
    orc = eu.oracle(num_speakers=6)
    ref, _ = eu.ref_encoder_batch(orc, ids_list)
    for b, L in enumerate(add_lens):
        ref[b, :L] += orc.w["speaker_embedding.weight"][spk[b]]
    eu.assert_encoder_close(got, ref, lens)
