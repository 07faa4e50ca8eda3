"""Helpers of the encoder contract tests (test_encoder_util_cpu.py, test_gpu_encoder_contract.py):
``tts_encoder_run_state`` called directly (any B with state, which no product method does), the
fp64 oracle as the reference of every sentence, and the comparator.

Bounds: the project's model-half tolerances (test_gpu_parity.py: mel relative RMS 4e-6, max-abs
4e-6 for bounded quantities).  The encoder's h lies in (-1, 1), so both apply to ``out`` and h_n;
c_n is unbounded and its max-abs scales with max(1, max|c_ref|).  They are not derived from what
the kernels give.  On the CPU the fp32 oracle sits at <= 1.5e-7 relative RMS and <= 1.1e-7 max-abs
of the fp64 oracle (profiles/encoder_contract.json), 25x under them."""
import ctypes
import os

import numpy as np

from conftest import golden, golden_flags, load_pkg, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle

MEL_RTOL = 4e-6    # == test_gpu_parity.MEL_RTOL (test_encoder_util_cpu.py checks it)
ALIGN_ATOL = 4e-6  # == test_gpu_parity.ALIGN_ATOL
EH = 256           # LSTM hidden size per direction

# tts_encoder_last_path
PATH_PER_STEP, PATH_RESIDENT, PATH_RESIDENT_BATCH = 0, 1, 2


class _env:
    """Environment variables for the duration of a with-block."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------- inputs
def sentence(L, k=0):
    """Ids of the k-th sentence of length L: one seed per (L, k), so two sentences of a batch never
    share ids, and cases that use the same (L, k) share one oracle run."""
    return weights_mod().synthetic_ids(int(L), 5000 + 64 * int(L) + int(k))


def sentences(lens):
    """One sentence per entry of ``lens``; the j-th of a repeated length gets k = j."""
    seen, out = {}, []
    for L in lens:
        k = seen.get(int(L), 0)
        seen[int(L)] = k + 1
        out.append(sentence(L, k))
    return out


def group_lens(B, seed=11):
    """B lengths from 1..24 (distinct while B <= 24, else each value used as evenly as 24 allow),
    with a length-1 sentence, the longest sentence not at index 0, and for B >= 16 the length-1
    sentence in the longest one's sentence group (the batched resident BiLSTM gives each XCD pair
    G = ceil(B / 4) consecutive sentences): that group's short sentences republish their last h
    for most of its steps."""
    rng = np.random.Generator(np.random.PCG64(seed + B))
    lens = np.concatenate([rng.permutation(np.arange(1, 25)) for _ in range((B + 23) // 24)])[:B]
    if 1 not in lens:
        lens[int(np.argmin(lens))] = 1
    if lens[0] == lens.max():
        t = max(k for k in range(B) if lens[k] < lens[0])
        lens[[0, t]] = lens[[t, 0]]
    i = int(np.argmax(lens))
    if B >= 16:
        G = (B + 3) // 4
        g0, g1 = (i // G) * G, min((i // G) * G + G, B)
        j = int(np.flatnonzero(lens == 1)[0])
        if not g0 <= j < g1:
            k = next(k for k in range(g0, g1) if lens[k] < lens[i])
            lens[[j, k]] = lens[[k, j]]
    return [int(x) for x in lens]


def dispatch_lens(Lmax):
    """64 sentences for the convolution dispatch by B * Lmax: one at Lmax (not at index 0), one each
    at the tile edges 16, 17, 32, 33, 64 that fit, the rest 1..12."""
    edges = [Lmax] + [x for x in (16, 17, 32, 33, 64) if x <= Lmax]
    rng = np.random.Generator(np.random.PCG64(100 + Lmax))
    lens = [int(x) for x in rng.integers(1, 13, size=64)]
    for k, x in enumerate(edges):
        lens[5 + 9 * k] = x  # spread over the sentence groups
    return lens


def pad_ids(ids_list, Lmax=None):
    lens = [len(x) for x in ids_list]
    Lmax = max(lens) if Lmax is None else Lmax
    ids = np.zeros((len(ids_list), Lmax), np.int32)
    for b, x in enumerate(ids_list):
        ids[b, :lens[b]] = x
    return ids, lens


def draw_state(B, seed):
    """Caller state [4][B][256] (h_fwd, h_bwd, c_fwd, c_bwd): h in (-0.9, 0.9), c in (-1, 1), every
    sentence and direction different."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h = rng.uniform(-0.9, 0.9, size=(2, B, EH))
    c = rng.uniform(-1.0, 1.0, size=(2, B, EH))
    return np.concatenate([h, c]).astype(np.float32)


def split_state(state):
    """[4][B][256] -> per sentence (h [2, 256], c [2, 256]), the oracle's ``state`` argument."""
    state = np.asarray(state)
    return [(state[0:2, b], state[2:4, b]) for b in range(state.shape[1])]


# ---------------------------------------------------------------------------- reference
_ORACLES = {}
_REF_CACHE = {}  # (id(oracle), ids bytes, state bytes) -> (oracle, out, (h_n, c_n))


def oracle(dtype=np.float64, **spec_kw):
    """The oracle on weights.tacotron2_weights(0) (the models' weights), one per dtype / spec."""
    key = (np.dtype(dtype).name, tuple(sorted(spec_kw.items())))
    if key not in _ORACLES:
        fl = golden_flags(golden("t2_fwdmask_L100"))
        _ORACLES[key] = Tacotron2Oracle(weights_mod().tacotron2_weights(0, **spec_kw), dtype=dtype, **fl)
    return _ORACLES[key]


def ref_encoder_batch(orc, ids_list, states=None):
    """Every sentence alone through ``orc.encoder``: (out [B, Lmax, 512] zero past L_b, state
    [4, B, 256] in the header's order).  ``states``: per sentence (h [2, 256], c [2, 256]) or None."""
    B, Lmax = len(ids_list), max(len(x) for x in ids_list)
    out = np.zeros((B, Lmax, 512), orc.dt)
    st = np.zeros((4, B, EH), orc.dt)
    for b, ids in enumerate(ids_list):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        s = None if states is None or states[b] is None else tuple(np.ascontiguousarray(v, dtype=np.float64)
                                                                   for v in states[b])
        key = (id(orc), ids.tobytes(), b"" if s is None else s[0].tobytes() + s[1].tobytes())
        if key not in _REF_CACHE:
            o, (hN, cN) = orc.encoder(ids, state=s, return_state=True)
            for v in (o, hN, cN):
                v.setflags(write=False)
            _REF_CACHE[key] = (orc, o, (hN, cN))  # (holds orc: its id is not reused)
        _, o, (hN, cN) = _REF_CACHE[key]
        out[b, :len(ids)] = o
        st[0:2, b] = hN
        st[2:4, b] = cN
    return out, st


# ---------------------------------------------------------------------------- comparator
def encoder_errors(got, ref, lens, got_state=None, ref_state=None):
    """Per-sentence figures of one comparison: relative RMS and max-abs of out (and of h_n, c_n),
    the count of nonzero (or NaN) elements past L_b, max|c_ref|."""
    got = np.asarray(got)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape and len(lens) == got.shape[0], (got.shape, ref.shape, len(lens))
    e = dict(out_rel=[], out_abs=[], pad_nonzero=[])
    for b, L in enumerate(lens):
        g = got[b, :L].astype(np.float64)
        e["out_rel"].append(rel_rms(g, ref[b, :L]))
        e["out_abs"].append(float(np.abs(g - ref[b, :L]).max()) if np.isfinite(g).all() else float("inf"))
        e["pad_nonzero"].append(int(np.count_nonzero(got[b, L:])))
    if ref_state is not None:
        gs = np.asarray(got_state).astype(np.float64)
        rs = np.asarray(ref_state, np.float64)
        assert gs.shape == rs.shape == (4, len(lens), EH), (gs.shape, rs.shape)
        for name, sl in (("h", slice(0, 2)), ("c", slice(2, 4))):
            e[name + "_rel"] = [rel_rms(gs[sl, b], rs[sl, b]) for b in range(len(lens))]
            e[name + "_abs"] = [float(np.abs(gs[sl, b] - rs[sl, b]).max()) if np.isfinite(gs[sl, b]).all()
                                else float("inf") for b in range(len(lens))]
        e["c_ref_max"] = [float(np.abs(rs[2:4, b]).max()) for b in range(len(lens))]
    return e


def assert_encoder_close(got, ref, lens, got_state=None, ref_state=None):
    """Every sentence: out within MEL_RTOL relative RMS and ALIGN_ATOL max-abs of the reference,
    rows past L_b exactly zero; with a state, h_n under the same two bounds and c_n under MEL_RTOL
    and ALIGN_ATOL * max(1, max|c_ref|).  Returns encoder_errors()."""
    assert (got_state is None) == (ref_state is None), "state given on one side only"
    e = encoder_errors(got, ref, lens, got_state, ref_state)
    for b, L in enumerate(lens):
        where = f"sentence {b} (L = {L})"
        assert e["out_rel"][b] < MEL_RTOL, f"{where}: out rel RMS {e['out_rel'][b]:.3e}"
        assert e["out_abs"][b] < ALIGN_ATOL, f"{where}: out max-abs {e['out_abs'][b]:.3e}"
        assert e["pad_nonzero"][b] == 0, f"{where}: {e['pad_nonzero'][b]} nonzero elements past L"
        if ref_state is not None:
            assert e["h_rel"][b] < MEL_RTOL, f"{where}: h_n rel RMS {e['h_rel'][b]:.3e}"
            assert e["h_abs"][b] < ALIGN_ATOL, f"{where}: h_n max-abs {e['h_abs'][b]:.3e}"
            assert e["c_rel"][b] < MEL_RTOL, f"{where}: c_n rel RMS {e['c_rel'][b]:.3e}"
            assert e["c_abs"][b] < ALIGN_ATOL * max(1.0, e["c_ref_max"][b]), \
                f"{where}: c_n max-abs {e['c_abs'][b]:.3e} (max|c_ref| {e['c_ref_max'][b]:.3f})"
    return e


# ---------------------------------------------------------------------------- device
def make_model(max_batch=64, resident=True, num_speakers=0, max_len=256):
    """Tacotron2 on weights.tacotron2_weights(0) with its native handles created: ``resident=False``
    creates them under TTS_RESIDENT=0 (read in tts_encoder_create, not per call), so every call on
    that handle takes the per-step launches."""
    t2 = load_pkg("tacotron2")
    fl = golden_flags(golden("t2_fwdmask_L100"))
    m = t2.Tacotron2(130, num_speakers, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                     forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                     forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"],
                     max_batch=max_batch, max_len=max_len)
    m.decoder.max_decoder_steps = 64  # (the decoder handle comes with the encoder's; keep it small)
    m = m.cuda().eval()
    if resident:
        m._handles(max_len, max_batch)
    else:
        with _env(TTS_RESIDENT=0):
            m._handles(max_len, max_batch)
    return m


def encoder_path(model):
    _native = load_pkg("_native")
    p = ctypes.c_int(-1)
    _native.check(_native.lib().tts_encoder_last_path(model._native[3], ctypes.byref(p)), "tts_encoder_last_path")
    return p.value


def run_encoder(model, ids_padded, lens, state_in=None, want_state=False, fill=float("nan")):
    """tts_encoder_run_state on the model's encoder handle.  ids_padded [B, Lmax] ints, lens [B],
    state_in [4, B, 256] or None.  Returns (out [B, Lmax, 512] fp32, state_out [4, B, 256] fp32 or
    None, tts_encoder_last_path).  The output buffers start as NaN: what the call leaves unwritten
    is seen."""
    import torch
    _native = load_pkg("_native")
    lib = _native.lib()
    ids_padded = np.asarray(ids_padded)
    B, Lmax = ids_padded.shape
    assert len(lens) == B and model._native is not None
    ids32 = torch.from_numpy(np.ascontiguousarray(ids_padded, dtype=np.int32)).cuda()
    out = torch.full((B, Lmax, 512), fill, device="cuda")
    st_in = None if state_in is None else torch.from_numpy(np.ascontiguousarray(state_in, dtype=np.float32)).cuda()
    assert st_in is None or tuple(st_in.shape) == (4, B, EH)
    st_out = torch.full((4, B, EH), fill, device="cuda") if want_state else None
    _native.check(lib.tts_encoder_run_state(
        model._native[3], ctypes.c_void_p(ids32.data_ptr()), _native.i32_array(lens), B, Lmax,
        ctypes.c_void_p(st_in.data_ptr()) if st_in is not None else None,
        ctypes.c_void_p(st_out.data_ptr()) if st_out is not None else None,
        ctypes.c_void_p(out.data_ptr()), _native.stream_handle()), "tts_encoder_run_state")
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if st_out is None else st_out.cpu().numpy(), encoder_path(model)


def add_speakers(model, enc, lens, speaker_ids):
    """tts_encoder_add_speakers on a host array [B, Lmax, 512]; returns the result."""
    import torch
    _native = load_pkg("_native")
    enc_d = torch.from_numpy(np.ascontiguousarray(enc, dtype=np.float32)).cuda()
    B, Lmax = enc_d.shape[0], enc_d.shape[1]
    _native.check(_native.lib().tts_encoder_add_speakers(
        model._native[3], ctypes.c_void_p(enc_d.data_ptr()), _native.i32_array(lens), _native.i32_array(speaker_ids),
        B, Lmax, _native.stream_handle()), "tts_encoder_add_speakers")
    torch.cuda.synchronize()
    return enc_d.cpu().numpy()


# ---------------------------------------------------------------------------- one checked call
RECORDS = []  # one entry per checked call (tools/encoder_contract_report.py writes them out)


def check_call(case, handle, model, ids_list, expect_path, Lmax=None, state_in=None, want_state=False,
               ref_state_in=None):
    """Run one call, record its figures, print them, then assert the serving path and the bounds
    against the fp64 oracle (started from ``ref_state_in`` where a chain of calls threads the
    oracle's own state, else from ``state_in``).  Returns (out, state_out, reference state_out)."""
    ids, lens = pad_ids(ids_list, Lmax)
    got, got_state, path = run_encoder(model, ids, lens, state_in, want_state)
    if ref_state_in is None:
        ref_state_in = state_in
    assert (ref_state_in is None) == (state_in is None)
    ref, ref_state = ref_encoder_batch(oracle(), ids_list, None if ref_state_in is None else split_state(ref_state_in))
    if ids.shape[1] > ref.shape[1]:  # Lmax above the longest sentence: zero rows
        ref = np.concatenate([ref, np.zeros((ref.shape[0], ids.shape[1] - ref.shape[1], 512))], axis=1)
    e = encoder_errors(got, ref, lens, got_state, ref_state if want_state else None)
    rec = dict(case=case, handle=handle, B=len(lens), Lmax=int(ids.shape[1]), path=path, expect_path=expect_path,
               state_in=state_in is not None, state_out=bool(want_state),
               **{k: max(v) for k, v in e.items() if k != "c_ref_max"})
    print("encoder contract:", rec)
    RECORDS.append(dict(rec, _ids=ids_list, _state=ref_state_in))
    assert path == expect_path, f"{case}: served by path {path}, expected {expect_path}"
    assert_encoder_close(got, ref, lens, got_state, ref_state if want_state else None)
    return got, got_state, ref_state
