"""GPU: the contract of tts_tacotron_encode (csrc/tacotron_api.hip: embedding gather + Prenet, the
K = 16 encoder CBHG, the speaker embedding, the GST reference encoder and style-token attention of
csrc/tacotron_kernels.hip), term by term against the fp64 oracle (tacotron_encoder_util.py):
 (a) the encoder term under the project's bounds and within 10x of the fp32 oracle's worst,
 (b) the speaker term enc(speaker) - enc(none) against the embedding row,
 (c) the style term enc(style) - enc(none) against the oracle's GST vector, on a model whose style
     weights are sharpened so that the style mel shows in it (on the shipped weights the GST vector
     is the same for every style to 1e-5; see the helper's docstring and its CPU tests, which hold
     a list of oracle mutants to a 10x margin at the shapes used here).
Ids past lens[b] are -1 / 0x7FFFFFFF, the output starts as a sentinel bit pattern and rows past
lens[b] must come back +0.0 bitwise.  Every call asserts the ConvKind of its eleven launches
(tts_tacotron_encode_last_path): 16-frame tiles up to 4096 frames, 64-frame tiles above; another
kernel on a healthy MI355X is a failure.  Three models serve every case.

Measured on an MI355X (profiles/tacotron_encoder_contract.json, worst sentence of any case;
relative RMS / max-abs), the fp32 oracle's figure on the same inputs in brackets:
  encoder term, 16- and 64-frame tiles  1.3e-7 / 3.2e-8  (8.9e-8 / 3.2e-8)   bound 9.0e-7 / 3.3e-7
  speaker term                          2.8e-8 / 3.0e-8  (2.7e-8 / 3.0e-8)   bound 2.8e-7 / 3.0e-7
  style term, sharpened weights         7.2e-7 / 1.0e-6  (3.6e-7 / 3.7e-7)   bound 3.6e-6 / 3.8e-6
  style term, shipped weights           2.0e-7 / 1.7e-8  (2.1e-7 / 2.2e-8)   bound 2.2e-6 / 2.3e-7
Every launch took the kind expected, every row past lens[b] came back +0.0, and every case passed
as the kernels stood: no kernel had to change."""
import numpy as np
import pytest
import torch

import tacotron_encoder_util as u
from tacotron_encoder_util import GSTM, INVALID, SHARP, TACO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    """The three models, made on first use and kept for the module."""
    made = {}

    def get(which):
        if which not in made:
            made[which] = u.make_model(which, max_batch=64)
        return made[which]
    return get


def _style_batch64():
    sp = u.specs(u.lens_b64_short(), 2)
    return sp, [(u.TS_BATCH, b) for b in range(64)]


# ============================================================================ encoder term
@pytest.mark.parametrize("L", u.LENS_B1)
@pytest.mark.parametrize("which", [GSTM, TACO])
def test_encoder_batch1_lengths(models, which, L):
    """Lengths below and across the 16-tap bank window (7 left, 8 right), the k = 3 halo, the pool
    partner and the 16-frame tiles, on the GST and the plain Tacotron model."""
    u.check_case(f"a_{which}_L{L}", which, models(which), u.specs([L]))


@pytest.mark.parametrize("lens,Lmax", u.RAGGED)
def test_encoder_ragged_lmax_above_longest(models, lens, Lmax):
    """Ragged batches under an Lmax above the longest sentence: padding ids that are no table rows
    are never gathered, rows past L come back +0.0, the backward GRU starts at L - 1."""
    u.check_case("b_" + "_".join(map(str, lens)) + f"_Lmax{Lmax}", GSTM, models(GSTM), u.specs(lens), Lmax=Lmax)


@pytest.mark.parametrize("total", [4098, 4096, 4097])
def test_encoder_64_frame_tiles(models, total):
    """64 sentences of 1, 63 .. 66, 127 .. 129 frames: 4098 and 4097 frames take the 64-frame tiles of
    KW = 1 / 3 / 16, 4096 frames still the 16-frame tiles; the lists differ in sentence 63 alone.
    Two sentences per length, so sixteen oracle runs serve the three cases."""
    lens = u.lens_tiled64(total)
    u.check_case(f"c_B64_{total}", GSTM, models(GSTM), u.specs(lens, 2))


# ============================================================================ speaker term
def test_speaker_term_batch5(models):
    """B = 5, speakers [3, 0, 2, 0, 1]: each sentence gets its own row, bounded by the rounding of
    the sum."""
    u.check_case("d_speakers", GSTM, models(GSTM), u.specs(u.LENS_B5), speakers=list(u.SPEAKERS))


def test_speaker_ids_change_nothing_without_speakers(models):
    """The num_speakers = 1 model ignores speaker ids, out-of-range ones included: bitwise."""
    u.check_case("d_taco_speakers", TACO, models(TACO), u.specs(u.LENS_B5), speakers=[3, 0, 99, -1, 1])


@pytest.mark.parametrize("bad", [4, -1])
def test_speaker_id_out_of_range(models, bad):
    ids, lens, Lmax = u.padded_ids(u.specs(u.LENS_B5))
    st, out = u.raw_encode(models(GSTM), ids, lens, Lmax, speakers=[3, 0, bad, 0, 1])
    assert st == INVALID and u.untouched(out)


# ============================================================================ style term
@pytest.mark.parametrize("Ts", u.STYLE_TS)
def test_style_batch1_lengths_sharpened(models, Ts):
    """style_frames with an odd height at each of the six stride-2 layers, H6 = 1, 2, 3, 4 rows into
    the GRU (one step up to 64 frames), on the sharpened weights."""
    u.check_case(f"e_sharp_Ts{Ts}", SHARP, models(SHARP), [u.STYLE_SENT], styles=[(Ts, 0)])


def test_style_per_sentence_batch5_and_broadcast(models):
    """Five styles for five sentences at Ts = 65; and one style given to encode() as [1, Ts, 80] is
    the explicit repeat, bitwise."""
    m = models(SHARP)
    sp = u.specs(u.LENS_B5)
    u.check_case("f_sharp_B5", SHARP, m, sp, styles=[(u.TS_BATCH, b) for b in range(5)])
    ids, lens, _ = u.padded_ids(sp)
    one = torch.from_numpy(np.array(u.style_of(u.TS_BATCH, 2)))
    a = m.encode(torch.from_numpy(ids), lens, style_mel=one[None])
    b = m.encode(torch.from_numpy(ids), lens, style_mel=one[None].repeat(5, 1, 1))
    assert u.encode_kinds(m)[10] == u.KIND_TILED16
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    st, raw = u.raw_encode(m, ids, lens, max(lens), style=np.stack([u.style_of(u.TS_BATCH, 2)] * 5))
    assert st == 0 and np.array_equal(raw.view(np.uint32), a.cpu().numpy().view(np.uint32))


def test_style_per_sentence_batch64(models):
    """B = 64 at Ts = 65, a style per sentence: sentences 0, 31 and 63 against the oracle, and every
    sentence's rows bitwise what a batch-1 call with its style returns (each workgroup of the GST
    kernels and each tile of the convolutions belongs to one sentence)."""
    m = models(SHARP)
    sp, styles = _style_batch64()
    outs = u.check_case("g_sharp_B64", SHARP, m, sp, styles=styles, check=(0, 31, 63))
    differ = []
    for b, (L, k) in enumerate(sp):
        ids, lens, Lmax = u.padded_ids([(L, k)])
        st, one = u.raw_encode(m, ids, lens, Lmax, style=u.style_of(*styles[b])[None])
        assert st == 0
        if not np.array_equal(one[0].view(np.uint32), outs["style"][b, :L].view(np.uint32)):
            differ.append((b, float(np.abs(one[0] - outs["style"][b, :L]).max())))
    print("sentences that differ from their batch-1 result:", differ)
    assert not differ


@pytest.mark.parametrize("Ts", u.STYLE_TS)
def test_style_batch1_lengths_shipped_weights(models, Ts):
    """The same lengths on the shipped weights.  A much weaker check: there the GST vector is the
    mean of the value rows whatever the style mel (over these lengths another style moves it by
    8e-7 .. 3.4e-5 and a dropped last row by 1e-6 .. 4e-6 at nine of the twelve, against a bound of
    2.2e-6), so this shows that the vector is right and little about the path from the style mel
    to it."""
    u.check_case(f"h_shipped_Ts{Ts}", GSTM, models(GSTM), [u.STYLE_SENT], styles=[(Ts, 0)])


# ============================================================================ one handle, many shapes
def test_one_handle_many_shapes(models):
    """Style 200 -> style 1 -> the B = 64 style batch -> 4097 frames without style -> style 200: the
    GST buffers g0 / g1 regrow and shrink in use, the sequence buffers grow under them; nothing
    stale shows and the last call is bitwise the first."""
    m = models(SHARP)
    first = u.check_case("i_1_Ts200", SHARP, m, [u.STYLE_SENT], styles=[(200, 0)])
    u.check_case("i_2_Ts1", SHARP, m, [u.STYLE_SENT], styles=[(1, 0)])
    sp, styles = _style_batch64()
    u.check_case("i_3_B64_Ts65", SHARP, m, sp, styles=styles, check=(0, 31, 63))
    u.check_case("i_4_B64_4097", SHARP, m, u.specs(u.lens_tiled64(4097), 2), check=(0, 31, 62, 63))
    last = u.check_case("i_5_Ts200", SHARP, m, [u.STYLE_SENT], styles=[(200, 0)])
    for name in ("none", "style"):
        assert np.array_equal(first[name].view(np.uint32), last[name].view(np.uint32)), name


# ============================================================================ argument contract
def test_invalid_arguments_leave_out_untouched(models):
    sp = u.specs((9, 17, 4))
    ids, lens, Lmax = u.padded_ids(sp, 21)
    style = np.stack([u.style_of(5, b) for b in range(3)])
    st, out = u.raw_encode(models(TACO), ids, lens, Lmax, style=style)  # style_mel on a non-GST model
    assert st == INVALID and u.untouched(out)
    m = models(SHARP)
    st, out = u.raw_encode(m, ids, lens, Lmax, style=style, style_frames=0)
    assert st == INVALID and u.untouched(out)
    st, out = u.raw_encode(m, ids, [9, 0, 4], Lmax)
    assert st == INVALID and u.untouched(out)
    st, out = u.raw_encode(m, ids, [9, 22, 4], Lmax)
    assert st == INVALID and u.untouched(out)
    ids65 = np.tile(ids[:1], (65, 1))
    st, out = u.raw_encode(m, ids65, [9] * 65, Lmax)  # B above the handle's 64
    assert st == INVALID and u.untouched(out)
    st, out = u.raw_encode(m, ids, lens, Lmax, style=style)  # and the handle still serves
    assert st == 0 and not u.untouched(out)


def test_encode_style_forms(models):
    """Through encode(): compute_style_mel's [1, 80, T] tensor is read as rows of 80 consecutive
    values, a 2-D style is one sentence's, and the shapes that cannot be are refused."""
    m = models(SHARP)
    sp = u.specs((9, 17, 4))
    ids, lens, Lmax = u.padded_ids(sp)
    idt = torch.from_numpy(ids)
    T = 33
    flat = np.array(u.style_of(T, 0))  # [T, 80]: the same memory seen as [1, 80, T]
    st, want = u.raw_encode(m, ids, lens, Lmax, style=np.stack([flat] * 3))
    assert st == 0
    for form in (torch.from_numpy(flat).reshape(1, 80, T), torch.from_numpy(flat), torch.from_numpy(flat)[None]):
        got = m.encode(idt, lens, style_mel=form)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), tuple(form.shape)
    with pytest.raises(ValueError, match="batch"):
        m.encode(idt, lens, style_mel=torch.from_numpy(flat)[None].repeat(2, 1, 1))
    with pytest.raises(ValueError, match="80-value rows"):
        m.encode(idt, lens, style_mel=torch.zeros(1, 81))
    with pytest.raises(TypeError):
        models(TACO).encode(idt, lens, style_mel=torch.from_numpy(flat))
