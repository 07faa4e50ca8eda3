"""Helpers of the Tacotron / TacotronGST encoder contract tests (test_tacotron_encoder_util_cpu.py,
test_gpu_tacotron_encoder_contract.py): ``tts_tacotron_encode`` called through ctypes on the
model's handle with padding ids that are no table rows and the output prefilled with a sentinel
bit pattern; the fp64 ``TacotronOracle`` as the reference of every sentence; oracle mutants that
say what the inputs can tell apart; and the comparator.

Three models: TacotronGST with 4 speakers and the plain Tacotron with one, both on the shipped
generator weights, and TacotronGST on *sharpened* style weights.  On the shipped weights the
style-token softmax is nearly uniform and the GST vector is the mean of the value rows whatever
the style mel is: under a speaker, another sentence's style moves the summed encoder output by
1.1e-6 .. 1.8e-6 relative RMS, inside the project's 4e-6 bound (pinned by the CPU test).  SHARPEN is the recipe, as
data: gst.* entries of a copy of ``weights.tacotron_gst_weights(0)`` multiplied by a factor,
loaded with ``load_state_dict`` and given to the oracle as well.

The output is three terms, each checked alone because the sum understates an error in a small
term (RMS: encoder 0.03 - 0.065, speaker row 0.297, GST 0.022 shipped):
 (a) encoder term, a call with neither speaker nor style: the project's model-half bounds
     (test_gpu_parity.py: relative RMS MEL_RTOL = 4e-6, max-abs ALIGN_ATOL x max(1, max|ref|)), and
     within 10x of the fp32 oracle's worst over the case list (ENC_F32_REL / ENC_F32_ABS below),
     so that a 1e-6 error cannot hide under a 4e-6 bound;
 (b) speaker term enc(speaker) - enc(none) of two device calls against the embedding row;
 (c) style term enc(style) - enc(none) of two device calls against the fp64 ``gst()`` vector.
The bounds of (b) and (c) are 10x what the fp32 oracle gives when it performs the same
subtraction (fp32 rounding of (h + ad1) + ad2 enters the difference), measured on the CPU over
the inputs of the GPU cases (test_tacotron_encoder_util_cpu.py re-measures them); the factor 10
covers summation order, the kernels' fma chains against numpy's pairwise sums.  None of the
constants comes from what the kernels give.

Measured, fp32 oracle against fp64 oracle, worst sentence over the inputs of the GPU cases
(encoder_inputs / style_inputs; relative RMS / max-abs), and the bounds, 10x:
  encoder term           8.9e-8 / 3.2e-8  -> ENC_REL, ENC_ABS     = 9.0e-7 / 3.3e-7
  speaker term           2.7e-8 / 3.0e-8  -> SPK_REL, SPK_ABS     = 2.8e-7 / 3.0e-7
  style term, sharpened  3.6e-7 / 3.7e-7  -> STYLE_REL, STYLE_ABS = 3.6e-6 / 3.8e-6
  style term, shipped    2.1e-7 / 2.2e-8  ->                        2.2e-6 / 2.3e-7
(the speaker term's error is the rounding of the sum alone: half an ulp of a value below 1).

Smallest movement of the style term by a GST mutant on the sharpened weights, over STYLE_TS and
the batches: 6.7e-4 relative RMS (drop_last_row at Ts = 200; next_style 9.2e-3), 186x the bound.
On the shipped weights another style moves the term by 8e-7 .. 3.4e-5 over STYLE_TS (1.5e-5 ..
2.4e-5 in the Ts = 65 batch, 7 - 11x its bound and short of the margin) and a dropped last row by
1e-6 .. 4e-6, the bound itself, at nine of the twelve lengths: the shipped-weight cases show
little more than that the term is the right constant vector."""
import ctypes

import numpy as np

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from oracle.tacotron_oracle import TacotronOracle, _sig, _softmax
from postnet_util import KIND_TILED16, KIND_TILED64, SENTINEL_BITS
from test_gpu_parity import ALIGN_ATOL, MEL_RTOL

GSTM, TACO, SHARP = "gst", "taco", "sharp"  # the three models
INVALID = 1  # TTS_ERR_INVALID
PAD_IDS = (-1, 0x7FFFFFFF)  # what the ids hold past lens[b], alternately: neither is a table row

# The sharpening: (gst.* key, factor).  W_query and W_key x 32 each take the style-token scores from
# ~1e-3 (a uniform softmax) to order 1, where the weights answer to h; W_value x 8 lifts the GST
# vector's RMS from 0.022 to 0.25 - 0.32, above the encoder output's, so that the fp32 rounding of
# the sum is a small part of the style term's bound.  Swept on the CPU over x 2 .. 32 (and the GRU
# input weights x 1 .. 4, which gained less than a factor 2 and are left alone): the smallest mutant
# movement grows with the factor up to 32 (6.7e-4 relative RMS, against 1.2e-5 at x 4).
SHARPEN = (("gst.style_token_layer.attention.W_query.weight", 32.0),
           ("gst.style_token_layer.attention.W_key.weight", 32.0),
           ("gst.style_token_layer.attention.W_value.weight", 8.0))

# fp32 oracle against the fp64 oracle over the inputs of the GPU cases (see the module docstring;
# test_tacotron_encoder_util_cpu.py re-measures them), and the bounds: 10x
ENC_F32_REL, ENC_F32_ABS = 9.0e-8, 3.3e-8
ENC_REL, ENC_ABS = 10 * ENC_F32_REL, 10 * ENC_F32_ABS
SPK_F32_REL, SPK_F32_ABS = 2.8e-8, 3.0e-8
SPK_REL, SPK_ABS = 10 * SPK_F32_REL, 10 * SPK_F32_ABS
STYLE_F32_REL = {SHARP: 3.6e-7, GSTM: 2.2e-7}
STYLE_F32_ABS = {SHARP: 3.8e-7, GSTM: 2.3e-8}
STYLE_REL = {k: 10 * v for k, v in STYLE_F32_REL.items()}
STYLE_ABS = {k: 10 * v for k, v in STYLE_F32_ABS.items()}

# ---------------------------------------------------------------------------- case lists
LENS_B1 = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33)
RAGGED = (((9, 17), 21), ((4, 33, 1, 16), 40), ((1,), 24))  # (lens, Lmax)
LENS_64 = (1, 63, 64, 65, 66, 127, 128, 129)
STYLE_TS = (1, 2, 3, 4, 5, 33, 63, 64, 65, 127, 128, 129, 200)
TS_BATCH = 65
SPEAKERS = (3, 0, 2, 0, 1)
LENS_B5 = (9, 17, 4, 33, 16)


def specs(lens, distinct=None):
    """(L, k) per entry of ``lens``: the j-th occurrence of a length gets k = j, or k = j mod
    ``distinct`` so that a 64-sentence batch needs ``distinct`` oracle runs per length."""
    seen, out = {}, []
    for L in lens:
        j = seen.get(int(L), 0)
        seen[int(L)] = j + 1
        out.append((int(L), j if distinct is None else j % distinct))
    return out


def lens_tiled64(total):
    """64 lengths drawn from LENS_64 with the sum ``total`` = 4096, 4097 or 4098.  Sentences 0..62
    are one seeded shuffle of 12 x 1, 23 x 63, 8 x 64, 5 x 65, 3 x 66, 4 x 127, 4 x 128, 4 x 129
    (4032 frames); sentence 63 has 64, 65 or 66 frames, so the lists differ in that sentence alone."""
    assert total in (4096, 4097, 4098)
    base = [1] * 12 + [63] * 23 + [64] * 8 + [65] * 5 + [66] * 3 + [127] * 4 + [128] * 4 + [129] * 4
    assert len(base) == 63 and sum(base) == 4032
    rng = np.random.Generator(np.random.PCG64(64))
    lens = [int(base[j]) for j in rng.permutation(63)] + [total - 4032]
    assert sum(lens) == total and set(lens) <= set(LENS_64)
    return lens


# ---------------------------------------------------------------------------- inputs
def ids_of(L, k=0):
    """The k-th sentence of L characters: weights.synthetic_ids, one seed per (L, k); read-only."""
    a = weights_mod().synthetic_ids(int(L), 5000 + 8 * int(L) + int(k))
    a.setflags(write=False)
    return a


_STYLES = {}


def style_of(Ts, k=0):
    """The k-th style mel of Ts frames: weights.synthetic_style_mel, one seed per (Ts, k)."""
    key = (int(Ts), int(k))
    if key not in _STYLES:
        m = weights_mod().synthetic_style_mel(key[0], 9000 + 64 * key[0] + key[1])
        m.setflags(write=False)
        _STYLES[key] = m
    return _STYLES[key]


# ---------------------------------------------------------------------------- weights, oracles
_SD, _ORACLES, _REFS = {}, {}, {}


def flags(which):
    return golden_flags(golden("taco_L12_softmax" if which == TACO else "gst_L10_nostyle"))


def state_dict(which):
    """The model's weights: tacotron_gst_weights(0, ...) with 4 speakers (GSTM), without GST and with
    one speaker (TACO), or without speakers and with SHARPEN applied to its gst.* entries (SHARP)."""
    if which not in _SD:
        w = weights_mod()
        if which == GSTM:
            sd = w.tacotron_gst_weights(0, num_speakers=4)
        elif which == TACO:
            sd = w.tacotron_gst_weights(0, num_speakers=1, gst=False)
        else:
            sd = w.tacotron_gst_weights(0)
            for part, f in SHARPEN:
                hit = [k for k in sd if part in k]
                assert hit and all(k.startswith("gst.") for k in hit), part
                for k in hit:
                    sd[k] = (sd[k] * np.float32(f)).astype(np.float32)
        _SD[which] = sd
    return _SD[which]


def oracle(which, dtype=np.float64):
    key = (which, np.dtype(dtype).name)
    if key not in _ORACLES:
        _ORACLES[key] = TacotronOracle(state_dict(which), **dict(flags(which), dtype=dtype))
    return _ORACLES[key]


def _cached(key, fn):
    if key not in _REFS:
        r = np.asarray(fn())
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def enc_ref(which, L, k=0, dtype=np.float64):
    """The encoder term of sentence (L, k): oracle.encoder(ids) [L, 256], no speaker, no style.  The
    encoder weights of the three models are the same arrays (one generator stream per key), so GSTM
    and SHARP share the entry."""
    w = TACO if which == TACO else GSTM
    return _cached(("enc", w, np.dtype(dtype).name, int(L), int(k)), lambda: oracle(w, dtype).encoder(ids_of(L, k)))


def gst_ref(which, Ts, k=0, dtype=np.float64):
    """oracle.gst(style_of(Ts, k)) [256]."""
    return _cached(("gst", which, np.dtype(dtype).name, int(Ts), int(k)),
                   lambda: oracle(which, dtype).gst(style_of(Ts, k)))


def spk_row(s):
    return np.asarray(state_dict(GSTM)["speaker_embedding.weight"][int(s)], np.float64)


def f32_term(which, L, k, add):
    """What an exact-to-fp32 implementation returns for the difference of the two calls:
    fp32(h + add) - h on the fp32 oracle's encoder output h, in fp64 as the comparator forms it."""
    h = enc_ref(which, L, k, np.float32)
    assert h.dtype == np.float32
    return (h + np.asarray(add, np.float32)[None, :]).astype(np.float64) - h.astype(np.float64)


def lens_b64_short():
    """The 64 sentences of the B = 64 style batch: LENS_B1 in turn (883 frames)."""
    return [LENS_B1[b % len(LENS_B1)] for b in range(64)]


STYLE_SENT = (17, 0)  # the sentence (L, k) of the batch-1 style cases


def encoder_inputs():
    """Every (model, L, k) whose encoder term a GPU case compares with the oracle."""
    s = {(w, L, 0) for w in (GSTM, TACO) for L in LENS_B1}
    for lens, _ in RAGGED:
        s |= {(GSTM, L, k) for L, k in specs(lens)}
    for total in (4096, 4097, 4098):
        s |= {(GSTM, L, k) for L, k in specs(lens_tiled64(total), 2)}
    s |= {(GSTM, L, k) for L, k in specs(LENS_B5)}
    s |= {(GSTM, L, k) for L, k in specs(lens_b64_short(), 2)}
    s.add((GSTM,) + STYLE_SENT)
    return sorted(s)


def style_inputs(which):
    """Every (L, k, Ts, ks) whose style term a GPU case compares with the oracle on model ``which``."""
    s = [STYLE_SENT + (Ts, 0) for Ts in STYLE_TS]
    if which == SHARP:
        s += [(L, k, TS_BATCH, b) for b, (L, k) in enumerate(specs(LENS_B5))]
        sp = specs(lens_b64_short(), 2)
        s += [sp[b] + (TS_BATCH, b) for b in (0, 31, 63)]
    return s


def f32_encoder(which, L, k):
    return vec_errors(enc_ref(which, L, k, np.float32), enc_ref(which, L, k))


def f32_speaker(L, k, s):
    return vec_errors(f32_term(GSTM, L, k, spk_row(s)), spk_row(s))


def f32_style(which, L, k, Ts, ks):
    return vec_errors(f32_term(which, L, k, gst_ref(which, Ts, ks, np.float32)), gst_ref(which, Ts, ks))


# ---------------------------------------------------------------------------- oracle mutants
# Each mutant is the oracle with one plausible kernel mistake.  CBHG mutants move the encoder term,
# GST mutants the style term; test_tacotron_encoder_util_cpu.py asserts that each moves its term by
# at least MARGIN times the term's bound at the shapes of the GPU cases, except where it is the
# identity (listed with the mutant).
MARGIN = 10.0
CBHG_MUTANTS = ("bank_pad_swap", "pool_prev", "k3_drop_last", "bwd_gru_lmax")
GST_MUTANTS = ("drop_last_row", "next_style", "hw_swap", "gru_rz_swap", "no_score_scale", "heads_interleaved",
               "no_tanh")


def h6_of(Ts):
    h = int(Ts)
    for _ in range(6):
        h = (h - 1) // 2 + 1
    return h


def mutant_is_identity(name, L=None, Lmax=None, Ts=None, B=None):
    """The shapes at which a mutant computes what the oracle computes (the only lawful exceptions
    of the margin condition):
      pool_prev, k3_drop_last  L = 1: the one frame has no partner and no halo frame;
      bwd_gru_lmax             Lmax = L: nothing past the sentence;
      drop_last_row            Ts = 1: no style is left to run (the mutant is undefined);
      next_style               B = 1: the next sentence is the sentence itself;
      hw_swap                  H6 = 1 (Ts <= 64): one row, the regrouping has nothing to swap."""
    if name in ("pool_prev", "k3_drop_last"):
        return L == 1
    if name == "bwd_gru_lmax":
        return Lmax == L
    if name == "drop_last_row":
        return Ts == 1
    if name == "next_style":
        return B == 1
    if name == "hw_swap":
        return h6_of(Ts) == 1
    return False


def cbhg_mutant(o, x, mut=None, Lmax=None):
    """TacotronOracle.cbhg of the encoder (K = 16, projections [128, 128]) with mistake ``mut``
    (None: the oracle's own arithmetic, bitwise):
      bank_pad_swap  members of even k padded [k/2, (k-1)/2] instead of [(k-1)/2, k/2];
      pool_prev      max(y[t], y[t-1]) with y[-1] = 0 instead of max(y[t], y[t+1]), y[L] = 0;
      k3_drop_last   the projections' right tap reads frame L-1 as zero (a halo filled for t < L-1);
      bwd_gru_lmax   the backward GRU starts at Lmax-1 over zero rows past L instead of at L-1."""
    prefix, K = "encoder.cbhg.cbhg", 16
    xt = x.T
    L = x.shape[0]
    outs = []
    for k in range(1, K + 1):
        pl, pr = (k - 1) // 2, k // 2
        if mut == "bank_pad_swap":
            pl, pr = pr, pl
        outs.append(o._bn_conv(f"{prefix}.conv1d_banks.{k - 1}", xt, k, pl, pr, "relu"))
    y = np.concatenate(outs, 0)
    if mut == "pool_prev":
        yp = np.pad(y, ((0, 0), (1, 0)))
        y = np.maximum(yp[:, 1:], yp[:, :-1])
    else:
        yp = np.pad(y, ((0, 0), (0, 1)))
        y = np.maximum(yp[:, :-1], yp[:, 1:])
    for i in range(2):
        p = f"{prefix}.conv1d_projections.{i}"
        if mut == "k3_drop_last":
            W = o.w[p + ".conv1d.weight"]
            yp = np.pad(y, ((0, 0), (1, 1)))
            yr = yp.copy()
            yr[:, L] = 0  # padded column L is frame L-1
            z = np.zeros((W.shape[0], L), o.dt)
            for j in range(3):
                z += W[:, :, j] @ (yr if j == 2 else yp)[:, j:j + L]
            z = o._bn(p + ".bn", z, 1e-3)
            y = np.maximum(z, 0) if i == 0 else z
        else:
            y = o._bn_conv(p, y, 3, 1, 1, "relu" if i == 0 else None)
    y = y.T + x
    for i in range(4):
        hp = f"{prefix}.highways.{i}"
        Hh = np.maximum(y @ o.w[hp + ".H.weight"].T + o.w[hp + ".H.bias"], 0)
        Tt = _sig(y @ o.w[hp + ".T.weight"].T + o.w[hp + ".T.bias"])
        y = Hh * Tt + y * (1.0 - Tt)
    fwd = o._gru_seq(f"{prefix}.gru", y, "")
    if mut == "bwd_gru_lmax":
        yl = np.concatenate([y, np.zeros((int(Lmax) - L, y.shape[1]), o.dt)], 0)
        bwd = o._gru_seq(f"{prefix}.gru", yl, "_reverse", reverse=True)[:L]
    else:
        bwd = o._gru_seq(f"{prefix}.gru", y, "_reverse", reverse=True)
    return np.concatenate([fwd, bwd], 1)


def encoder_mutant(which, L, k, mut=None, Lmax=None):
    o = oracle(TACO if which == TACO else GSTM)
    x = o._prenet("encoder.prenet", o.w["embedding.weight"][ids_of(L, k)])
    return cbhg_mutant(o, x, mut, Lmax)


def gst_mutant(o, style, mut=None, next_style=None):
    """TacotronOracle.gst with mistake ``mut`` (None: the oracle's own arithmetic, bitwise):
      drop_last_row      the style mel without its last row;
      next_style         the style mel of the batch's next sentence;
      hw_swap            each channel's [H6, W6] plane read as if stored [W6, H6];
      gru_rz_swap        the GRU's reset and update gate rows exchanged;
      no_score_scale     scores not divided by key_dim ** 0.5 = 8;
      heads_interleaved  head h = units h, h + 4, ... instead of the contiguous 64;
      no_tanh            the style tokens used without tanh."""
    w = o.w
    if mut == "drop_last_row":
        style = style[:-1]
    elif mut == "next_style":
        style = next_style
    x = np.asarray(style, o.dt)[None]
    for i in range(6):
        W, b = w[f"gst.encoder.convs.{i}.weight"], w[f"gst.encoder.convs.{i}.bias"]
        _, Hh, Ww = x.shape
        Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
        y = np.zeros((W.shape[0], Ho, Wo), o.dt)
        for ki in range(3):
            for kj in range(3):
                patch = xp[:, ki:ki + 2 * (Ho - 1) + 1:2, kj:kj + 2 * (Wo - 1) + 1:2]
                y += np.einsum("oc,chw->ohw", W[:, :, ki, kj], patch)
        y += b[:, None, None]
        x = np.maximum(o._bn(f"gst.encoder.bns.{i}", y, 1e-5), 0)
    if mut == "hw_swap":
        C, H6, W6 = x.shape
        x = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(C, H6, W6)
    seq = x.transpose(1, 0, 2).reshape(x.shape[1], -1)
    if mut == "gru_rz_swap":
        p = [w[f"gst.encoder.recurrence.{n}_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        H = p[1].shape[1]
        perm = np.concatenate([np.arange(H, 2 * H), np.arange(0, H), np.arange(2 * H, 3 * H)])
        p = [a[perm] for a in p]
        h = np.zeros(H, o.dt)
        for t in range(seq.shape[0]):
            h = o._gru_cell(seq[t], h, *p)
    else:
        h = o._gru_seq("gst.encoder.recurrence", seq)[-1]
    tokens = w["gst.style_token_layer.style_tokens"]
    if mut != "no_tanh":
        tokens = np.tanh(tokens)
    q = w["gst.style_token_layer.attention.W_query.weight"] @ h
    keys = tokens @ w["gst.style_token_layer.attention.W_key.weight"].T
    vals = tokens @ w["gst.style_token_layer.attention.W_value.weight"].T
    out = np.zeros(256, o.dt)
    for hd in range(4):
        sl = slice(hd, 256, 4) if mut == "heads_interleaved" else slice(64 * hd, 64 * hd + 64)
        s = keys[:, sl] @ q[sl]
        p = _softmax(s if mut == "no_score_scale" else s / 8.0)
        out[sl] = p @ vals[:, sl]
    return out


def vec_errors(got, ref):
    """(relative RMS, max-abs) of a [L, 256] term against a [256] vector on every row, or of two
    arrays of one shape."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if ref.ndim == 1 and got.ndim == 2:
        ref = np.broadcast_to(ref[None, :], got.shape)
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    return rel_rms(got, ref), float(np.abs(got - ref).max())


# ---------------------------------------------------------------------------- comparator
def pad_out(arrays, Lmax=None):
    """Per-sentence [L_b, 256] -> fp32 [B, Lmax, 256] as the device call returns it (zero rows)."""
    Lmax = max(len(a) for a in arrays) if Lmax is None else Lmax
    out = np.zeros((len(arrays), Lmax, 256), np.float32)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out


def pad_bad(got, lens):
    """Per sentence: elements past lens[b] that are not +0.0 (bitwise: -0.0, NaN, the sentinel count)."""
    return [int(np.count_nonzero(np.ascontiguousarray(got[b, L:]).view(np.uint32))) for b, L in enumerate(lens)]


def term_errors(got, lens, refs):
    """Per-sentence figures of a [B, Lmax, 256] array (an output, or a difference of two outputs in
    fp64) against per-sentence references ([L, 256], or [256] for every row): relative RMS,
    max-abs, max|ref|, NaN count of the valid rows."""
    e = dict(rel=[], abs=[], ref_max=[], nan=[])
    for b, (L, r) in enumerate(zip(lens, refs)):
        g = np.asarray(got[b, :L], np.float64)
        rel, ab = vec_errors(g, r)
        e["rel"].append(rel)
        e["abs"].append(ab)
        e["ref_max"].append(float(np.abs(r).max()))
        e["nan"].append(int(np.isnan(g).sum()))
    return e


def assert_encoder_term(got, lens, refs, what="encoder term"):
    """(a): no NaN; the project's bounds; within 10x of the fp32 oracle's worst; zero rows past L."""
    assert got.dtype == np.float32 and got.shape[0] == len(lens) and got.shape[2] == 256, got.shape
    e = term_errors(got, lens, refs)
    bad = pad_bad(got, lens)
    for b, L in enumerate(lens):
        where = f"{what}, sentence {b} (L = {L})"
        assert e["nan"][b] == 0, f"{where}: {e['nan'][b]} NaN in valid rows"
        assert e["rel"][b] < MEL_RTOL, f"{where}: rel RMS {e['rel'][b]:.3e}"
        assert e["abs"][b] < ALIGN_ATOL * max(1.0, e["ref_max"][b]), f"{where}: max-abs {e['abs'][b]:.3e}"
        assert e["rel"][b] <= ENC_REL, f"{where}: rel RMS {e['rel'][b]:.3e} above 10x the fp32 oracle's {ENC_F32_REL:.1e}"
        assert e["abs"][b] <= ENC_ABS, f"{where}: max-abs {e['abs'][b]:.3e} above 10x the fp32 oracle's {ENC_F32_ABS:.1e}"
        assert bad[b] == 0, f"{where}: {bad[b]} elements past L not +0.0"
    return e


def assert_added_term(with_add, without, lens, vecs, rel_bound, abs_bound, what):
    """(b) / (c): the difference of two device outputs (fp64) against a vector per sentence."""
    diff = with_add.astype(np.float64) - without.astype(np.float64)
    e = term_errors(diff, lens, vecs)
    bad = pad_bad(with_add, lens)
    for b, L in enumerate(lens):
        where = f"{what}, sentence {b} (L = {L})"
        assert e["nan"][b] == 0, f"{where}: {e['nan'][b]} NaN in valid rows"
        assert e["rel"][b] <= rel_bound, f"{where}: rel RMS {e['rel'][b]:.3e} above {rel_bound:.1e}"
        assert e["abs"][b] <= abs_bound, f"{where}: max-abs {e['abs'][b]:.3e} above {abs_bound:.1e}"
        assert bad[b] == 0, f"{where}: {bad[b]} elements past L not +0.0"
    return e


# ---------------------------------------------------------------------------- device
def make_model(which, max_batch=64):
    """The model ``which`` on the device, decoder cap small; SHARP loads its state dict."""
    import torch
    t = load_pkg("tacotron")
    fl = flags(which)
    cls = t.Tacotron if which == TACO else t.TacotronGST
    m = cls(130, {GSTM: 4, TACO: 1, SHARP: 0}[which], r=fl["r"], memory_size=fl["memory_size"],
            attn_win=fl["attn_win"], attn_norm=fl["attn_norm"], forward_attn=fl["forward_attn"],
            trans_agent=fl["trans_agent"], forward_attn_mask=fl["forward_attn_mask"],
            location_attn=fl["location_attn"], max_batch=max_batch)
    m.decoder.max_decoder_steps = 20
    if which == SHARP:
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state_dict(SHARP).items()})
    else:
        for k, v in state_dict(which).items():  # the generator's weights are the oracle's
            assert np.array_equal(m.state_dict()[k].numpy(), v), k
    return m.cuda().eval()


def padded_ids(sp, Lmax=None):
    """int32 [B, Lmax]: sentence b's ids, then PAD_IDS alternately."""
    lens = [L for L, _ in sp]
    Lmax = max(lens) if Lmax is None else Lmax
    assert Lmax >= max(lens)
    a = np.empty((len(sp), Lmax), np.int32)
    a[:, 0::2] = PAD_IDS[0]
    a[:, 1::2] = PAD_IDS[1]
    for b, (L, k) in enumerate(sp):
        a[b, :L] = ids_of(L, k)
    return a, lens, Lmax


def sentinel(shape):
    import torch
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def encode_kinds(model):
    _native = load_pkg("_native")
    kinds = (ctypes.c_int * 11)()
    _native.check(_native.lib().tts_tacotron_encode_last_path(model._native[0], kinds, 11),
                  "tts_tacotron_encode_last_path")
    return [int(x) for x in kinds]


def expect_kinds(frames, style):
    """TILED16 up to 4096 frames, TILED64 above; the GST projection (B x H6 <= 4096 rows in every
    case here) on the 16-frame tiles, -1 without a style."""
    k = KIND_TILED16 if frames <= 4096 else KIND_TILED64
    return [k] * 10 + [KIND_TILED16 if style else -1]


def raw_encode(model, ids, lens, Lmax, speakers=None, style=None, style_frames=None, B=None):
    """tts_tacotron_encode through ctypes on the model's handle.  ids: int32 [B, Lmax] array; style:
    fp32 [B, Ts, 80] array or None.  The output starts as the sentinel.  Returns (status, out
    [B, Lmax, 256] fp32 numpy)."""
    import torch
    _native = load_pkg("_native")
    B = len(lens) if B is None else B
    lib, h = model._handle(min(Lmax, model.max_len), min(B, model.max_batch), need_steps=1)
    ids_d = torch.from_numpy(np.array(ids, np.int32)).cuda()
    out = sentinel((max(B, len(lens)), Lmax, 256))
    sm = None
    if style is not None:
        sm = torch.from_numpy(np.array(style, np.float32)).cuda()
        style_frames = sm.shape[1] if style_frames is None else style_frames
    st = lib.tts_tacotron_encode(
        h, ctypes.c_void_p(ids_d.data_ptr()), _native.i32_array(lens), B, Lmax,
        _native.i32_array(speakers) if speakers is not None else None,
        ctypes.c_void_p(sm.data_ptr()) if sm is not None else None, int(style_frames or 0),
        ctypes.c_void_p(out.data_ptr()), _native.stream_handle())
    torch.cuda.synchronize()
    return int(st), out.cpu().numpy()


def untouched(out):
    return bool((out.view(np.uint32) == SENTINEL_BITS).all())


# ---------------------------------------------------------------------------- one checked case
RECORDS = []  # one entry per checked case (tools/tacotron_encoder_contract_report.py writes them out)


def _worst(e):
    return dict(rel=max(e["rel"]), abs=max(e["abs"]))


def check_case(case, which, model, sp, Lmax=None, speakers=None, styles=None, check=None):
    """One case on the (L, k) sentences ``sp``: the call without speaker and style is held to (a);
    with ``speakers`` a second call is held to (b); with ``styles`` (a (Ts, k) per sentence) a
    further call without speakers is held to (c).  ``check``: the sentences whose encoder term is
    compared with the oracle (default all; the others are still checked for zero rows).  Every
    call asserts its kinds.  Prints and records the figures before asserting.  Returns the outputs
    (none, speaker, style)."""
    ids, lens, Lmax = padded_ids(sp, Lmax)
    frames = sum(lens)
    rec = dict(case=case, model=which, B=len(sp), Lmax=Lmax, frames=frames, kinds={}, _sp=list(sp), _styles=styles,
               _speakers=speakers, _check=check)
    outs, kinds = {}, {}
    st, outs["none"] = raw_encode(model, ids, lens, Lmax)
    assert st == 0, f"{case}: status {st}"
    kinds["none"] = encode_kinds(model)
    if speakers is not None:
        st, outs["speaker"] = raw_encode(model, ids, lens, Lmax, speakers=speakers)
        assert st == 0, f"{case}: status {st} with speakers"
        kinds["speaker"] = encode_kinds(model)
    if styles is not None:
        sm = np.stack([style_of(Ts, k) for Ts, k in styles])
        st, outs["style"] = raw_encode(model, ids, lens, Lmax, style=sm)
        assert st == 0, f"{case}: status {st} with style"
        kinds["style"] = encode_kinds(model)
    rec["kinds"] = kinds
    sel = list(range(len(sp))) if check is None else list(check)
    sub = lambda a: a[sel]
    sl = [lens[b] for b in sel]
    refs = [enc_ref(which, *sp[b]) for b in sel]
    rec["encoder"] = _worst(term_errors(sub(outs["none"]), sl, refs))
    rec["pad_bad"] = {k: sum(pad_bad(v, lens)) for k, v in outs.items()}
    if speakers is not None and which == GSTM:
        d = outs["speaker"].astype(np.float64) - outs["none"].astype(np.float64)
        rec["speaker"] = _worst(term_errors(d, lens, [spk_row(s) for s in speakers]))
    if styles is not None:
        d = outs["style"].astype(np.float64) - outs["none"].astype(np.float64)
        rec["style"] = _worst(term_errors(sub(d), sl, [gst_ref(which, *styles[b]) for b in sel]))
    print("tacotron encoder contract:", {k: v for k, v in rec.items() if not k.startswith("_")})
    RECORDS.append(rec)
    for name, kk in kinds.items():
        want = expect_kinds(frames, name == "style")
        assert kk == want, f"{case} ({name}): launches served by kinds {kk}, expected {want}"
    assert_encoder_term(sub(outs["none"]), sl, refs)
    for name, o in outs.items():
        assert sum(pad_bad(o, lens)) == 0, f"{case} ({name}): {pad_bad(o, lens)} elements past L not +0.0"
    if speakers is not None:
        if which == GSTM:
            assert_added_term(outs["speaker"], outs["none"], lens, [spk_row(s) for s in speakers], SPK_REL, SPK_ABS,
                              "speaker term")
        else:
            assert np.array_equal(outs["speaker"].view(np.uint32), outs["none"].view(np.uint32)), \
                f"{case}: speaker ids changed the output of a model without speakers"
    if styles is not None:
        assert_added_term(sub(outs["style"]), sub(outs["none"]), sl, [gst_ref(which, *styles[b]) for b in sel],
                          STYLE_REL[which], STYLE_ABS[which], "style term")
    return outs
