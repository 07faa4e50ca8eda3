"""Oracle parity of the resident TacotronGST decoder (csrc/tacotron_resident.hip) at the edges of its three
splits: attention slices of 32 encoder positions, XCD groups of 4 sentences, mel rows m0 = r + 32 w / m1 = m0 + 256
with the memory queue's shift; and of the multi-launch path where the resident one ends.

Cases, inputs, the float64 reference (the numpy oracle's decoder on the same float32 encoder rows) and
check_sentence are tests/tacotron_resident_util.py's; tests/test_tacotron_resident_util_cpu.py shows on the CPU that
every case is decisive (each stop decision >= 1e-3 from 0.6), crosses the boundary it names, and that check_sentence
rejects a lost boundary hand-off, a tail read from the wrong index, a normaliser short of a slice, zeroed mel rows
from 256 on and swapped lengths.  Bounds: tests/test_gpu_tacotron.py's (step counts, stop decisions and the argmax
of every step that is no near tie of the oracle's exact; alignments and stop values max-abs 4e-6; mel relative
RMS 4e-6).

Measured on an MI355X (profiles/tacotron_resident_contract.json, tools/tacotron_resident_report.py) over every case:
alignment max-abs <= 6.0e-7 (r = 4, memory_size = 4), stop <= 7.4e-8, mel relative RMS <= 5.3e-8, at most 2.4 % of a
sentence's steps left out of the argmax comparison (L = 256: 12 of 501), every step count the oracle's; the first
B >= 2 sentences of the group-shape batch bitwise their B = 32 results.
"""
import numpy as np
import pytest

import tacotron_resident_util as u

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    """One model per (r, memory_size, serving path, constructor extras), made on first use."""
    cache = {}

    def get(r=5, m=5, path="default", **kw):
        key = (r, m, path, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = u.make_model(r, m, 200, **kw)
        return cache[key]
    return get


def _run(models, name, path="default", fill=0.0, first=None, only=None):
    """The case's batch (its first `first` sentences, or sentence `only` alone) on the device, on the serving
    path asked for (TTS_RESIDENT is read when a handle is created, so it stays set over the run); the path that
    served it must be the one the case table names."""
    c = u.CASES[name]
    sents = c["sents"][only:only + 1] if only is not None else c["sents"][:first]
    mp = pytest.MonkeyPatch()
    try:
        if path == "off":
            mp.setenv("TTS_RESIDENT", "0")
        res = u.run(models(c["r"], c["m"], path, **c["model_kw"]), sents, c["cap"], fill)
    finally:
        mp.undo()
    assert res["resident"] is (c["resident"] and path == "default"), f"{name}: served by the other path"
    return res


def _check(res, b, name, i):
    return u.check_sentence(u.sentence(res, b), u.case_reference(name, i), u.CASES[name]["sents"][i].L)


def _ids(name):
    return [f"L{s.L}" + (f"x{s.c:g}" if s.c != 1.0 else "") + f"_b{i}" for i, s in enumerate(u.CASES[name]["sents"])]


# ------------------------------------------------------------------ a. slice edges
@pytest.fixture(scope="module")
def edges(models):
    n = len(u.CASES["slice_edges"]["sents"])
    return dict(batch=_run(models, "slice_edges"), single=[_run(models, "slice_edges", only=i) for i in range(n)])


@pytest.mark.parametrize("i", range(len(u.EDGE_LENS)), ids=_ids("slice_edges"))
def test_slice_edges_in_a_batch(edges, i):
    """L on both sides of the boundaries 32, 64, 96 (and 1, 2) in one batch: three groups, the last of two."""
    assert edges["batch"]["lens"] == list(u.EDGE_LENS)
    _check(edges["batch"], i, "slice_edges", i)


@pytest.mark.parametrize("i", range(len(u.EDGE_LENS)), ids=_ids("slice_edges"))
def test_slice_edges_alone(edges, i):
    _check(edges["single"][i], 0, "slice_edges", i)


# ------------------------------------------------------------------ b. all seven boundaries
@pytest.fixture(scope="module")
def long_run(models):
    return _run(models, "long")


@pytest.mark.parametrize("i", [0, 1], ids=_ids("long"))
def test_all_seven_boundaries(long_run, i):
    """L = 255 and 256 to the reference's own 500-step cap: the attention crosses position 224 near step 446."""
    assert long_run["steps"] == [501, 501]
    _check(long_run, i, "long", i)


# ------------------------------------------------------------------ c. tail stop beyond slice 0
@pytest.fixture(scope="module")
def tail_runs(models):
    return {name: _run(models, name) for name in ("tail", "tail129")}


@pytest.mark.parametrize("name,i", [(n, i) for n in ("tail", "tail129") for i in range(len(u.CASES[n]["sents"]))],
                         ids=[f"{n}-{s}" for n in ("tail", "tail129") for s in _ids(n)])
def test_tail_stop_beyond_slice_0(tail_runs, name, i):
    """The alignment-tail rule fires from local index 31, 0, 31, 0, 0 of slices 0, 1, 1, 2, 4 at the oracle's
    step, and the unmodified slot-mates of the finished sentences go on to the cap unharmed."""
    c = u.CASES[name]
    res = tail_runs[name]
    if c["sents"][i].c != 1.0:
        assert res["steps"][i] <= c["cap"], "ended by the cap, not by the tail rule"
        assert res["steps"][i] < max(res["steps"]), "no slot-mate outlived the tail sentence"
    else:
        assert res["steps"][i] == c["cap"] + 1
    _check(res, i, name, i)


# ------------------------------------------------------------------ d. group shapes
@pytest.fixture(scope="module")
def groups(models):
    return {B: _run(models, "groups", first=B) for B in u.GROUP_BS}


@pytest.mark.parametrize("B", [B for B in u.GROUP_BS if 1 < B < 32])
def test_group_shapes_match_the_full_batch_bitwise(groups, B):
    """The first B sentences of the fixed 32 as a batch of their own (partial last groups of 1, 2, 3 sentences,
    one to eight groups): every sentence carries the bits it has in the B = 32 run (measured so on an MI355X for
    every B >= 2).  Sentence b keeps slot b % 4 of group b / 4, every reduction of the kernel runs in a fixed
    per-sentence order, and neither the number of sentences of its group nor the number of groups enters one."""
    full = groups[32]
    for b in range(B):
        L = u.GROUP_LENS[b]
        assert u.same_bits(u.sentence(groups[B], b), u.sentence(full, b), L), f"sentence {b} (L = {L})"


def test_group_shape_batch_1_matches_the_full_batch(groups):
    """B = 1 is not bitwise the sentence's B = 32 result, and no reduction of the resident kernel is the reason:
    the go frame's prenet layer 1 runs ahead of the kernel as a GEMM launch (tacotron_api.hip, enqueue_prenet_go),
    and sgemm.hip serves B = 1 with its VALU dot products (sgemm_kernel<0>) and B >= 2 with MFMA tiles, which
    sum K in another order.  The kernel's first input differs in its last bits, so the sentence is held to
    check_sentence's bounds against its B = 32 result (and to the oracle in test_slice_edges_alone)."""
    L = u.GROUP_LENS[0]
    fig = u.check_sentence(u.sentence(groups[1], 0), u.trimmed(u.sentence(groups[32], 0), L), L)
    assert fig["steps"] == u.CASES["groups"]["cap"] + 1


@pytest.mark.parametrize("i", u.CASES["groups"]["oracle"])
def test_group_slots_vs_oracle(groups, i):
    """Slots 0, 1, 2, 3 of groups 0, 2, 4 and 7 of the B = 32 run."""
    _check(groups[32], i, "groups", i)


# ------------------------------------------------------------------ e. mel rows and queue
@pytest.fixture(scope="module", params=u.MEL_PAIRS, ids=lambda p: f"r{p[0]}m{p[1]}")
def mel_runs(request, models):
    name = "mel_r%dm%d" % request.param
    return dict(name=name, batch=_run(models, name), single=_run(models, name, only=0))


@pytest.mark.parametrize("b", [-1, 0, 1, 2, 3, 4], ids=["alone"] + [f"b{i}_L{L}" for i, L in enumerate(u.MEL_LENS)])
def test_mel_rows_and_queue(mel_runs, b):
    """nmel = 320 and 480 put the m1 < nmel cut inside the second row block, (4, 5) and (1, 5) shift the queue by
    80 and 320 values; L = 40 moves 99.5 % of the attention mass past position 32 within the 100 steps."""
    name = mel_runs["name"]
    if b < 0:
        _check(mel_runs["single"], 0, name, 0)
    else:
        _check(mel_runs["batch"], b, name, b)


# ------------------------------------------------------------------ f. where the resident path ends
@pytest.mark.parametrize("name", ["b33", "L257", "queue560", "b32_L256"])
def test_where_the_resident_path_ends(models, name):
    """B = 33, L = 257 and a queue of 560 values run multi-launch, B = 32 with L = 256 still resident
    (asserted in _run); either way the sentences are the oracle's."""
    res = _run(models, name)
    for i in u.CASES[name]["oracle"]:
        _check(res, i, name, i)


# ------------------------------------------------------------------ g. capacity below the kernel's slices
def test_handle_smaller_than_the_slices(models):
    """max_batch = 4, max_len = 40 and a full batch: slices 2..7 start past the handle's rows (the initial
    boundary alpha of such a slice is not loaded: tacotron_resident.hip's setup)."""
    res = _run(models, "small_handle")
    m = models(**u.CASES["small_handle"]["model_kw"])
    assert m._native[1][1:] == (40, 4)
    for i in range(4):
        _check(res, i, "small_handle", i)


# ------------------------------------------------------------------ h. padding rows of enc
@pytest.fixture(scope="module")
def padded(models):
    return {(path, name): _run(models, "slice_edges", path=path, fill=fill)
            for path in ("default", "off") for name, fill in (("zero", 0.0), ("nan", float("nan")), ("1e30", 1e30))}


@pytest.mark.parametrize("fill", ["nan", "1e30"])
@pytest.mark.parametrize("path", ["default", "off"])
def test_padding_rows_of_enc_are_never_read(padded, path, fill):
    """Rows j >= lens[b] of enc may hold anything (include/tts_hip.h, tts_tacotron_decode): the outputs are
    bitwise those of the zero-padded batch, on both serving paths."""
    got, want = padded[path, fill], padded[path, "zero"]
    assert got["steps"] == want["steps"] and got["frames"] == want["frames"]
    assert np.array_equal(got["mel"], want["mel"])
    for b, L in enumerate(u.EDGE_LENS):
        assert u.same_bits(u.sentence(got, b), u.sentence(want, b), L), f"sentence {b} (L = {L})"
        assert np.all(got["align"][b, :got["steps"][b], L:] == 0)


def test_multilaunch_zero_padded_batch_vs_oracle(padded):
    """The multi-launch side of the padding case is itself the oracle's (two sentences)."""
    for i in (4, 9):
        _check(padded["off", "zero"], i, "slice_edges", i)
