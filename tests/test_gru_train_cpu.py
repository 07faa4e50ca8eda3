"""CPU: the float64 restatement of tests/gru_train_util.py against the gru_train.npz fixture (the reference's GRU
modules with autograd, float32 and float64), the condition that makes the GPU test's bound meetable, four mutants
that show the comparison can fail, and the surface of layers.GRU / use_device_gru that needs no GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import decoder_train_util as du
import gru_train_util as gu
from conftest import REPO, golden, load_pkg

F64_AGREE = 1e-12  # restatement against the reference's float64 run, in the bound's form: summation order only
SYMBOLS = ("tts_gru_create", "tts_gru_destroy", "tts_gru_set_weights", "tts_gru_reserve_floats", "tts_gru_forward",
           "tts_gru_backward")


@pytest.fixture(scope="module")
def fixture():
    return golden("gru_train")


@pytest.fixture(scope="module")
def meta(fixture):
    return json.loads(str(fixture["meta"]))


@pytest.fixture(scope="module")
def restated():
    return {case: gu.restate(gu.inputs(case)) for case in gu.CASES}


def test_bound_is_the_projects_and_the_reference_figures_leave_4e_6_deciding(meta):
    assert (gu.TOL, gu.MARGIN) == (du.TOL, du.MARGIN) == (4e-6, 4.0)
    ref32 = meta["reference_fp32"]
    assert sorted(ref32) == sorted(list(gu.CASES) + ["swap"])
    for case, figures in ref32.items():
        for name in figures:
            assert gu.tolerance(ref32, case, name) == gu.TOL, (case, name, figures[name])


def test_chunk_case_crosses_one_chunk_and_ends_partial():
    rows = gu.CASES["chunks"]["B"] * gu.CASES["chunks"]["T"]
    assert rows // gu.KC == 1 and rows % gu.KC
    src = open(os.path.join(REPO, "your-voice-tts_amd", "csrc", "gru_train.hip")).read()
    assert int(re.search(r"constexpr int GT_KC = (\d+);", src).group(1)) == gu.KC


def test_the_cases_reach_what_they_name():
    c = gu.CASES
    assert (c["one"]["B"], c["one"]["T"]) == (1, 1) and {c["t2"]["T"], c["t3"]["T"]} == {2, 3}
    assert c["b17"]["B"] == 17 and c["small"]["H"] % 32 and c["h16"]["H"] == 16
    gst, both = gu.inputs("gst"), gu.inputs("both_ups")
    assert gst["up_out"] is None and gst["up_hn"] is not None and not gst["bi"] and gst["I"] == 256
    assert both["up_out"] is not None and both["up_hn"] is not None
    assert gu.inputs("state")["h0"] is not None and gu.inputs("t24")["h0"] is None


@pytest.mark.parametrize("case", list(gu.CASES))
def test_restatement_agrees_with_the_reference_float64(case, fixture, restated):
    for name in gu.tensor_names(gu.CASES[case]["bi"]):
        full = restated[case][name]
        v = gu.ratio(gu.stored(case, name, full), fixture[gu.key(case, name, 64)], scale=np.abs(full).max())
        assert v <= F64_AGREE, f"{case} {name}: {v:.3e}"


@pytest.mark.parametrize("case", list(gu.CASES))
def test_reference_float32_lies_within_the_bound(case, fixture, restated, meta):
    for name in gu.tensor_names(gu.CASES[case]["bi"]):
        full = restated[case][name]
        v = gu.check(fixture[gu.key(case, name, 32)], gu.stored(case, name, full), f"{case} {name}",
                     scale=np.abs(full).max())
        assert v <= meta["reference_fp32"][case][name] * (1 + 1e-6) + 1e-12  # the stored figure is over the whole tensor


@pytest.mark.parametrize("mutant, case, tensor", [
    ("bias_hn_same", "t24", "grad_bias_hh_l0"), ("bias_hn_same", "t24", "grad_weight_hh_l0_reverse"),
    ("no_carry", "t24", "grad_x"), ("rev_index", "t3", "out"), ("hn_grad_dropped", "gst", "grad_x"),
    ("hn_grad_dropped", "both_ups", "grad_weight_ih_l0")])
def test_mutants_leave_the_bound(mutant, case, tensor, restated):
    """Each deliberate error is at least 100x outside the bound on the named tensor of the named case."""
    bad = gu.restate(gu.inputs(case), mutant=mutant)
    v = gu.ratio(bad[tensor], restated[case][tensor])
    print(f"{mutant} {case} {tensor}: {v:.3e}")
    assert v >= 100 * gu.TOL
    if mutant == "bias_hn_same":  # it touches nothing but the two W_hh-side gradients
        for name in ("out", "grad_x", "grad_bias_ih_l0", "grad_weight_ih_l0"):
            assert np.array_equal(bad[name], restated[case][name])


# ------------------------------------------------------------------ module surface
def test_state_dict_is_the_fixtures_and_loads_both_ways(meta):
    layers = load_pkg("layers")
    for which, (_, I, H, bi) in (("cbhg.gru", gu.SITES[0]), ("recurrence", gu.SITES[1])):
        ours, theirs = layers.GRU(I, H, batch_first=True, bidirectional=bi), nn.GRU(I, H, 1, batch_first=True,
                                                                                   bidirectional=bi)
        a = ours.state_dict()
        assert {k: list(v.shape) for k, v in a.items()} == meta["state_dict"][which]
        assert list(a) == list(theirs.state_dict()) == gu.param_names(bi)
        k = 1.0 / np.sqrt(H)
        assert all(float(v.abs().max()) <= k and float(v.abs().max()) > 0.5 * k for v in a.values())
        theirs.load_state_dict(a)
        assert all(torch.equal(theirs.state_dict()[n], a[n]) for n in a)
        ours.load_state_dict(nn.GRU(I, H, batch_first=True, bidirectional=bi).state_dict())
        ours.flatten_parameters()
        assert ours.repacks == 0 and ours.last_reserve_floats == 0


@pytest.mark.parametrize("kw, names", [
    (dict(num_layers=2), "num_layers"), (dict(batch_first=False), "batch_first"), (dict(bias=False), "bias"),
    (dict(dropout=0.1), "dropout"), (dict(dtype=torch.float64), "dtype"), (dict(input_size=24), "input_size"),
    (dict(hidden_size=40), "hidden_size"), (dict(hidden_size=144), "hidden_size")])
def test_unsupported_constructor_arguments_raise_and_name_the_argument(kw, names):
    layers = load_pkg("layers")
    args = dict(input_size=32, hidden_size=48, batch_first=True)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=names):
        layers.GRU(**args)


def test_batch_first_defaults_to_false_as_in_torch_and_so_raises():
    with pytest.raises(NotImplementedError, match="batch_first"):
        load_pkg("layers").GRU(32, 48)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_cpu_tensor_raises_no_gpu():
    m = load_pkg("layers").GRU(32, 48, batch_first=True, bidirectional=True)
    with pytest.raises(RuntimeError, match="no GPU"):
        m(torch.zeros(2, 3, 32))


def test_packed_sequence_is_not_implemented():
    m = load_pkg("layers").GRU(32, 48, batch_first=True)
    with pytest.raises(NotImplementedError, match="PackedSequence"):
        m(nn.utils.rnn.pack_padded_sequence(torch.zeros(2, 3, 32), [3, 2], batch_first=True))


def test_symbols_are_declared_and_bound():
    n = load_pkg("_native")
    header = open(os.path.join(REPO, "include", "tts_hip.h")).read()
    lib = n.load_library()
    for s in SYMBOLS:
        assert s in n.EXPORTS, s
        assert re.search(r"\b(tts_status|void|int64_t)\s+" + s + r"\s*\(", header), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.tts_gru_reserve_floats.restype is ctypes.c_int64


def test_use_device_gru_finds_exactly_the_reference_sites(meta):
    layers = load_pkg("layers")
    model = gu.tiny_model().eval()
    sites = [tuple(s) for s in meta["gru_sites"]]
    assert sites == list(gu.SITES) == gu.gru_sites(model)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert layers.use_device_gru(model) is model
    swapped = [(path, m.input_size, m.hidden_size, m.bidirectional) for path, m in model.named_modules()
               if isinstance(m, layers.GRU)]
    assert swapped == sites and not any(type(m) is nn.GRU for m in model.modules())
    assert not any(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    kept = [m for m in model.modules() if isinstance(m, layers.GRU)]
    layers.use_device_gru(model)  # idempotent: the same module objects stay
    assert [m for m in model.modules() if isinstance(m, layers.GRU)] == kept
    assert "optimizer afterwards" in layers.use_device_gru.__doc__


def test_use_device_gru_leaves_other_grus_alone():
    layers = load_pkg("layers")
    others = [nn.GRU(20, 32, batch_first=True), nn.GRU(32, 32, 2, batch_first=True), nn.GRU(32, 32),
              nn.GRU(32, 256, batch_first=True), nn.GRU(32, 32, batch_first=True, bias=False),
              nn.GRU(32, 32, batch_first=True).double()]
    model = nn.Sequential(*others, nn.GRU(32, 32, batch_first=True).train())
    layers.use_device_gru(model)
    assert all(model[i] is m for i, m in enumerate(others))
    assert isinstance(model[len(others)], layers.GRU) and model[len(others)].training


def test_c_abi_rejects_before_any_launch():
    """UNSUPPORTED sizes at create; INVALID (null pointers, weights not set) from the calls: none touches the GPU."""
    n = load_pkg("_native")
    lib = n.load_library()
    h = ctypes.c_void_p()
    for I, H in ((24, 48), (32, 40), (32, 144), (0, 48), (32, 0)):
        assert lib.tts_gru_create(I, H, 1, ctypes.byref(h)) == 3
    assert lib.tts_gru_create(32, 48, 1, None) == 1
    assert lib.tts_gru_create(32, 48, 1, ctypes.byref(h)) == 0
    assert lib.tts_gru_reserve_floats(h, 2, 3) == 2 * 3 * 2 * 48 * 4
    assert lib.tts_gru_reserve_floats(h, 0, 3) == 0 and lib.tts_gru_reserve_floats(None, 2, 3) == 0
    p16 = ctypes.c_void_p(16)
    assert lib.tts_gru_forward(h, None, 2, 3, None, None, None, None, None) == 1
    assert lib.tts_gru_forward(h, p16, 2, 3, None, p16, None, None, None) == 1  # weights not set
    assert lib.tts_gru_backward(h, p16, 2, 3, p16, p16, None, p16, None, None, None, None, None, None, None) == 1
    assert lib.tts_gru_set_weights(h, None, None, None, None, None) == 1
    lib.tts_gru_destroy(h)
    lib.tts_gru_destroy(None)


def test_use_device_gru_keeps_requires_grad_and_swaps_a_root_gru():
    layers = load_pkg("layers")
    model = nn.Sequential(nn.GRU(32, 32, batch_first=True, bidirectional=True))
    model[0].weight_hh_l0.requires_grad_(False)
    model[0].bias_ih_l0_reverse.requires_grad_(False)
    want = {n: p.requires_grad for n, p in model[0].named_parameters()}
    layers.use_device_gru(model)
    assert isinstance(model[0], layers.GRU) and {n: p.requires_grad for n, p in model[0].named_parameters()} == want
    root = nn.GRU(32, 32, batch_first=True).eval()
    swapped = layers.use_device_gru(root)
    assert isinstance(swapped, layers.GRU) and not swapped.training
    assert all(torch.equal(swapped.state_dict()[k], v) for k, v in root.state_dict().items())
    assert layers.use_device_gru(swapped) is swapped
    other = nn.GRU(20, 20)
    assert layers.use_device_gru(other) is other
