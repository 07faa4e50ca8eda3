"""Helpers of the Postnet / PostCBHG contract tests (test_postnet_util_cpu.py,
test_gpu_postnet_contract.py): ``tts_postnet_run`` called directly and ``tts_tacotron_postnet``
through ``Tacotron*.postnet``, with input rows past T_b set to NaN and the output prefilled with a
sentinel bit pattern; the fp64 oracles as the reference of every sentence; and the comparator.

Bounds: the project's model-half tolerances, imported from test_gpu_parity.py (relative RMS 4e-6,
max-abs 4e-6 x max(1, max|ref|)), applied per sentence to the output and, for Tacotron2, to the
postnet term ``out - mel`` alone (computed in fp64): with U[0, 1) inputs the term's RMS is 0.10
against 0.58 for the output, so an error in the term is understated about sixfold in the output.
They are not derived from what the kernels give.  On the CPU the fp32 oracle sits at <= 4.6e-7
(term) relative RMS of the fp64 one for T = 1..1040 and the PostCBHG linear at <= 4.9e-8 relative
RMS, 8.6e-8 max-abs for T = 1..300: a correct fp32 implementation has at least 7x room."""
import ctypes

import numpy as np

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from encoder_util import _env, make_model  # noqa: F401  (re-exported for the tests)
from oracle.tacotron2_oracle import Tacotron2Oracle
from oracle.tacotron_oracle import TacotronOracle
from test_gpu_parity import ALIGN_ATOL, MEL_RTOL

N_MEL, N_LIN = 80, 1025
T2, GST = "t2", "gst"  # tts_postnet_run / tts_tacotron_postnet

# ConvKind (csrc/conv1d.h), what tts_postnet_last_path reports per layer
(KIND_SMALL_CM, KIND_SMALL_TAP32, KIND_SMALL_TAP16, KIND_TILED16, KIND_SPLITK_REDUCE, KIND_SPLITK_FUSED,
 KIND_VARLEN64, KIND_TILED32, KIND_TILED64) = range(9)

# what the output holds before the call: a quiet NaN with a payload no kernel produces
SENTINEL_BITS = 0x7FC0BEEF


# ---------------------------------------------------------------------------- inputs
_MELS = {}


def mel(T, k=0):
    """The k-th mel of T frames: seeded U[0, 1) fp32 [T, 80] (the teacher-mel distribution of
    tests/golden/make_golden.py), one seed per (T, k); read-only."""
    key = (int(T), int(k))
    if key not in _MELS:
        rng = np.random.Generator(np.random.PCG64(7000 + 64 * key[0] + key[1]))
        m = rng.uniform(0.0, 1.0, size=(key[0], N_MEL)).astype(np.float32)
        m.setflags(write=False)
        _MELS[key] = m
    return _MELS[key]


def specs(lens):
    """(T, k) per entry of ``lens``; the j-th of a repeated length gets k = j, so no two sentences
    of a batch share frames and cases that use the same (T, k) share one oracle run."""
    seen, out = {}, []
    for T in lens:
        k = seen.get(int(T), 0)
        seen[int(T)] = k + 1
        out.append((int(T), k))
    return out


def _away_from_0(lens):
    """The longest sentence not at index 0."""
    lens = [int(x) for x in lens]
    if lens[0] == max(lens):
        j = max(i for i in range(len(lens)) if lens[i] < lens[0])
        lens[0], lens[j] = lens[j], lens[0]
    return lens


def lens_tiled16():
    """Case d: 64 sentences of 16..33 frames holding the tile edges 16, 17, 32, 33."""
    rng = np.random.Generator(np.random.PCG64(41))
    lens = [int(x) for x in rng.integers(17, 34, size=64)]
    for j, x in enumerate((16, 17, 32, 33)):
        lens[7 + 13 * j] = x
    return _away_from_0(lens)


def lens_varlen():
    """Case e: 64 sentences of 58..70 frames holding 63, 64, 65, the sum 4100 (just above 4096)."""
    rng = np.random.Generator(np.random.PCG64(42))
    lens = [int(x) for x in rng.integers(58, 71, size=64)]
    for j, x in enumerate((63, 64, 65)):
        lens[4 + 19 * j] = x
    fixed = {4, 23, 42}
    j = 0
    while sum(lens) != 4100:  # move the free sentences one frame at a time, inside 58..70
        if j not in fixed:
            step = 1 if sum(lens) < 4100 else -1
            if 58 <= lens[j] + step <= 70:
                lens[j] += step
        j = (j + 1) % 64
    return _away_from_0(lens)


def lens_cbhg64():
    """PostCBHG: 32 sentences holding 63, 64, 65, 129, the rest 130..142 with the sum 4100."""
    rng = np.random.Generator(np.random.PCG64(43))
    lens = [int(x) for x in rng.integers(130, 143, size=32)]
    for j, x in enumerate((63, 64, 65, 129)):
        lens[3 + 8 * j] = x
    fixed = {3, 11, 19, 27}
    j = 0
    while sum(lens) != 4100:
        if j not in fixed:
            step = 1 if sum(lens) < 4100 else -1
            if 130 <= lens[j] + step <= 142:
                lens[j] += step
        j = (j + 1) % 32
    return _away_from_0(lens)


# ---------------------------------------------------------------------------- reference
_ORACLES = {}
_REFS = {}  # (which, dtype, T, k) -> read-only reference


def oracle(which, dtype=np.float64):
    """Tacotron2Oracle on weights.tacotron2_weights(0) / TacotronOracle on tacotron_gst_weights(0)
    (the models' weights), one per dtype."""
    key = (which, np.dtype(dtype).name)
    if key not in _ORACLES:
        if which == T2:
            fl = golden_flags(golden("t2_fwdmask_L100"))
            _ORACLES[key] = Tacotron2Oracle(weights_mod().tacotron2_weights(0), dtype=dtype, **fl)
        else:
            fl = golden_flags(golden("gst_L10_nostyle"))
            _ORACLES[key] = TacotronOracle(weights_mod().tacotron_gst_weights(0), **dict(fl, dtype=dtype))
    return _ORACLES[key]


def out_dim(which):
    return N_MEL if which == T2 else N_LIN


def ref(which, T, k=0, dtype=np.float64):
    """``oracle(which, dtype).postnet(mel(T, k))``: [T, 80] mel_post or [T, 1025] linear; cached."""
    key = (which, np.dtype(dtype).name, int(T), int(k))
    if key not in _REFS:
        r = np.zeros((0, out_dim(which)), dtype) if T == 0 else np.asarray(oracle(which, dtype).postnet(mel(T, k)))
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def ref_batch(which, sp, dtype=np.float64):
    return [ref(which, T, k, dtype) for T, k in sp]


def pad_out(which, arrays, Tmax=None, fill=None):
    """Per-sentence results [T_b, C] -> one fp32 array [B, Tmax, C] as the device call returns it:
    rows past T_b hold the sentinel (tts_postnet_run) or zero (tts_tacotron_postnet)."""
    Tmax = max(1, max(len(a) for a in arrays)) if Tmax is None else Tmax
    out = np.zeros((len(arrays), Tmax, out_dim(which)), np.float32)
    if which == T2 and fill is None:
        out.view(np.uint32)[:] = SENTINEL_BITS
    elif fill is not None:
        out[:] = fill
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return out


# ---------------------------------------------------------------------------- comparator
def postnet_errors(which, got, mels, refs):
    """Per-sentence figures of one call: relative RMS and max-abs of the valid rows, max|ref|, for
    Tacotron2 the relative RMS of the postnet term out - mel (fp64), the count of NaN in valid rows
    and of elements past T_b that are not the sentinel (bitwise) / not zero."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.ndim == 3 and got.shape[0] == len(mels) == len(refs), got.shape
    assert got.shape[2] == out_dim(which)
    e = dict(out_rel=[], out_abs=[], ref_max=[], nan=[], pad_bad=[])
    if which == T2:
        e["term_rel"] = []
    for b, (m, r) in enumerate(zip(mels, refs)):
        T = len(m)
        assert r.shape == (T, out_dim(which)) and T <= got.shape[1], (b, r.shape, got.shape)
        g = got[b, :T].astype(np.float64)
        r = np.asarray(r, np.float64)
        ok = bool(np.isfinite(g).all())
        e["nan"].append(int(np.isnan(g).sum()))
        e["out_rel"].append(rel_rms(g, r) if T and ok else (0.0 if ok else float("inf")))
        e["out_abs"].append((float(np.abs(g - r).max()) if T else 0.0) if ok else float("inf"))
        e["ref_max"].append(float(np.abs(r).max()) if T else 0.0)
        if which == T2:
            m64 = np.asarray(m, np.float64)
            e["term_rel"].append(rel_rms(g - m64, r - m64) if T and ok else (0.0 if ok else float("inf")))
            e["pad_bad"].append(int(np.count_nonzero(got[b, T:].view(np.uint32) != SENTINEL_BITS)))
        else:
            e["pad_bad"].append(int(np.count_nonzero(got[b, T:].view(np.uint32))))  # (-0.0 and NaN count too)
    return e


def assert_postnet_close(which, got, mels, refs):
    """Every sentence: no NaN in a valid row; output (and, for Tacotron2, the postnet term) within
    MEL_RTOL relative RMS; max-abs within ALIGN_ATOL * max(1, max|ref|); rows past T_b bitwise the
    sentinel (tts_postnet_run never writes them) or exactly zero (tts_tacotron_postnet).  Returns
    postnet_errors()."""
    e = postnet_errors(which, got, mels, refs)
    for b, m in enumerate(mels):
        where = f"sentence {b} (T = {len(m)})"
        assert e["nan"][b] == 0, f"{where}: {e['nan'][b]} NaN in valid rows"
        assert e["out_rel"][b] < MEL_RTOL, f"{where}: out rel RMS {e['out_rel'][b]:.3e}"
        if which == T2:
            assert e["term_rel"][b] < MEL_RTOL, f"{where}: postnet term rel RMS {e['term_rel'][b]:.3e}"
        assert e["out_abs"][b] < ALIGN_ATOL * max(1.0, e["ref_max"][b]), \
            f"{where}: out max-abs {e['out_abs'][b]:.3e} (max|ref| {e['ref_max'][b]:.3f})"
        what = "not the sentinel" if which == T2 else "nonzero"
        assert e["pad_bad"][b] == 0, f"{where}: {e['pad_bad'][b]} elements past T {what}"
    return e


# ---------------------------------------------------------------------------- device
def make_gst_model(max_batch=64):
    """TacotronGST on weights.tacotron_gst_weights(0) under gst_L10_nostyle's flags, decoder cap small."""
    t = load_pkg("tacotron")
    fl = golden_flags(golden("gst_L10_nostyle"))
    m = t.TacotronGST(130, fl["num_speakers"], r=fl["r"], memory_size=fl["memory_size"], attn_win=fl["attn_win"],
                      attn_norm=fl["attn_norm"], forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                      forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"],
                      max_batch=max_batch)
    m.decoder.max_decoder_steps = 20
    return m.cuda().eval()


def _device_mel(mels, Tmax):
    """[B, Tmax, 80] on the device: sentence b's frames, NaN in every row past T_b."""
    import torch
    Tlong = max(1, max(len(m) for m in mels))
    Tmax = Tlong if Tmax is None else Tmax
    assert Tmax >= Tlong
    x = np.full((len(mels), Tmax, N_MEL), np.nan, np.float32)
    for b, m in enumerate(mels):
        x[b, :len(m)] = m
    return torch.from_numpy(x).cuda(), Tmax


def _sentinel(shape):
    import torch
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def postnet_kinds(model):
    _native = load_pkg("_native")
    kinds = (ctypes.c_int * 5)()
    _native.check(_native.lib().tts_postnet_last_path(model._native[1], kinds, 5), "tts_postnet_last_path")
    return [int(x) for x in kinds]


def run_postnet(model, mels, Tmax=None):
    """tts_postnet_run on the model's postnet handle (model._native[1]).  mels: [T_b, 80] arrays.
    Input rows past T_b are NaN up to Tmax; the output starts as the sentinel.  Returns (out
    [B, Tmax, 80] fp32, the five kinds of tts_postnet_last_path)."""
    import torch
    _native = load_pkg("_native")
    assert model._native is not None
    x, Tmax = _device_mel(mels, Tmax)
    out = _sentinel((len(mels), Tmax, N_MEL))
    _native.check(_native.lib().tts_postnet_run(
        model._native[1], ctypes.c_void_p(x.data_ptr()), _native.i32_array([len(m) for m in mels]), len(mels), Tmax,
        ctypes.c_void_p(out.data_ptr()), _native.stream_handle()), "tts_postnet_run")
    torch.cuda.synchronize()
    return out.cpu().numpy(), postnet_kinds(model)


def run_postcbhg(model, mels, Tmax=None):
    """``Tacotron*.postnet(mel, frames)`` (tts_tacotron_postnet) with NaN input rows past T_b.  The
    method allocates its own output with torch.empty; a tensor of that size filled with the
    sentinel is released just before, so that the caching allocator hands the same block back and
    rows the call left unwritten show as the sentinel, not as a stale zero.  Returns (linear
    [B, Tmax, 1025], whether the output did land on the prefilled block)."""
    import torch
    x, Tmax = _device_mel(mels, Tmax)
    pre = _sentinel((len(mels), Tmax, N_LIN))
    torch.cuda.synchronize()
    ptr = pre.data_ptr()
    del pre
    lin = model.postnet(x, [len(m) for m in mels])
    torch.cuda.synchronize()
    assert tuple(lin.shape) == (len(mels), Tmax, N_LIN)
    return lin.cpu().numpy(), lin.data_ptr() == ptr


# ---------------------------------------------------------------------------- one checked call
RECORDS = []  # one entry per checked call (tools/postnet_contract_report.py writes them out)


def check_call(case, which, model, sp, expect_kinds=None, Tmax=None):
    """Run one call on the (T, k) sentences ``sp``, record its figures, print them, then assert the
    kinds that served the five layers (Tacotron2) and the bounds against the fp64 oracle.  Returns
    the device output."""
    mels = [mel(T, k) for T, k in sp]
    if which == T2:
        (got, kinds), prefilled = run_postnet(model, mels, Tmax), True
    else:
        (got, prefilled), kinds = run_postcbhg(model, mels, Tmax), None
    refs = ref_batch(which, sp)
    e = postnet_errors(which, got, mels, refs)
    rec = dict(case=case, model=which, B=len(sp), Tmax=int(got.shape[1]), frames=int(sum(T for T, _ in sp)),
               Tlong=int(max(T for T, _ in sp)), kinds=kinds, expect_kinds=expect_kinds, prefilled=bool(prefilled),
               **{k: (sum(v) if k in ("nan", "pad_bad") else max(v)) for k, v in e.items() if k != "ref_max"})
    print("postnet contract:", rec)
    RECORDS.append(dict(rec, _specs=list(sp)))
    if expect_kinds is not None:
        assert kinds == list(expect_kinds), f"{case}: layers served by kinds {kinds}, expected {list(expect_kinds)}"
    assert_postnet_close(which, got, mels, refs)
    return got
