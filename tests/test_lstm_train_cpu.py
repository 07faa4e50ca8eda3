"""CPU: the float64 restatement of tests/lstm_train_util.py against the lstm_train.npz fixture (the reference's
nn.LSTM with autograd, float32 and float64), the condition that makes the GPU test's bound meetable, three
mutants that show the comparison can fail, and the surface of layers.LSTM that needs no GPU."""
import numpy as np
import pytest
import torch
from torch import nn

import encoder_util as eu
import lstm_train_util as lu
from conftest import golden, load_pkg

F64_AGREE = 1e-12  # restatement against the reference's float64 run, in the bound's form: summation order only


@pytest.fixture(scope="module")
def fixture():
    return golden("lstm_train")


@pytest.fixture(scope="module")
def restated():
    return {case: lu.restate(lu.inputs(case)) for case in lu.CASES}


def test_bound_is_the_projects():
    assert lu.TOL == eu.ALIGN_ATOL == 4e-6


def test_chunk_case_crosses_two_chunks_and_ends_partial():
    total = sum(lu.CASES["chunks"]["lens"])
    assert total // lu.KC == 2 and total % lu.KC


@pytest.mark.parametrize("case", list(lu.CASES))
def test_restatement_agrees_with_the_reference_float64(case, fixture, restated):
    for name in lu.tensor_names(lu.CASES[case]["bi"]):
        v = lu.ratio(lu.stored(case, name, restated[case][name]), fixture[lu.key(case, name, 64)])
        assert v <= F64_AGREE, f"{case} {name}: {v:.3e}"


@pytest.mark.parametrize("case", list(lu.CASES))
def test_reference_float32_lies_within_the_bound(case, fixture, restated):
    for name in lu.tensor_names(lu.CASES[case]["bi"]):
        lu.check(fixture[lu.key(case, name, 32)], fixture[lu.key(case, name, 64)], f"{case} {name} (fixture)")
        lu.check(fixture[lu.key(case, name, 32)], lu.stored(case, name, restated[case][name]), f"{case} {name}")


def test_padding_rows_are_zero_in_the_reference(fixture, restated):
    inp, r = lu.inputs("unsorted"), restated["unsorted"]
    for b, L in enumerate(inp["lens"]):
        assert not r["out"][b, L:].any() and not r["grad_x"][b, L:].any()


@pytest.mark.parametrize("mutant, case", [("no_carry", "packed"), ("rev_index", "unsorted"), ("bias_pad", "unsorted")])
def test_mutants_leave_the_bound(mutant, case, restated):
    """Each deliberate error is at least 100x outside the bound on at least one tensor."""
    bad = lu.restate(lu.inputs(case), mutant=mutant)
    worst = max(lu.ratio(bad[n], restated[case][n]) for n in lu.tensor_names(True))
    print(f"{mutant}: worst ratio {worst:.3e}")
    assert worst >= 100 * lu.TOL


# ------------------------------------------------------------------ module surface
def test_state_dict_matches_nn_lstm_and_loads_both_ways():
    layers = load_pkg("layers")
    for bi in (True, False):
        ours, theirs = layers.LSTM(32, 48, batch_first=True, bidirectional=bi), \
            nn.LSTM(32, 48, num_layers=1, batch_first=True, bidirectional=bi)
        a, b = ours.state_dict(), theirs.state_dict()
        assert list(a) == list(b) == lu.param_names(bi)
        assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
        k = 1.0 / np.sqrt(48)
        assert all(float(v.abs().max()) <= k and float(v.abs().max()) > 0.5 * k for v in a.values())
        theirs.load_state_dict(a)
        assert all(torch.equal(theirs.state_dict()[n], a[n]) for n in a)
        ours.load_state_dict(nn.LSTM(32, 48, batch_first=True, bidirectional=bi).state_dict())
        ours.flatten_parameters()


@pytest.mark.parametrize("kw", [dict(num_layers=2), dict(batch_first=False), dict(bias=False), dict(dropout=0.1),
                                dict(proj_size=8), dict(dtype=torch.float64), dict(input_size=24),
                                dict(hidden_size=40)])
def test_unsupported_constructor_arguments_raise(kw):
    layers = load_pkg("layers")
    args = dict(input_size=32, hidden_size=48, batch_first=True)
    args.update(kw)
    with pytest.raises(NotImplementedError):
        layers.LSTM(**args)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_cpu_tensor_raises_no_gpu():
    layers = load_pkg("layers")
    m = layers.LSTM(32, 48, batch_first=True, bidirectional=True)
    with pytest.raises(RuntimeError, match="no GPU"):
        m(torch.zeros(2, 3, 32))
    with pytest.raises(RuntimeError, match="no GPU"):
        m.lstm(torch.zeros(2, 3, 32), [3, 1])


def test_use_device_lstm_swaps_the_encoder_lstm():
    layers = load_pkg("layers")
    model = lu.tiny_model()
    before = {k: v.clone() for k, v in model.encoder.lstm.state_dict().items()}
    assert layers.use_device_lstm(model) is model and isinstance(model.encoder.lstm, layers.LSTM)
    after = model.encoder.lstm.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_c_abi_rejects_before_any_launch():
    """UNSUPPORTED sizes at create; INVALID (null pointers, weights not set) from the calls: none touches the GPU."""
    import ctypes
    n = load_pkg("_native")
    lib = n.load_library()
    h = ctypes.c_void_p()
    assert lib.tts_lstm_create(24, 48, 1, ctypes.byref(h)) == 3
    assert lib.tts_lstm_create(32, 40, 1, ctypes.byref(h)) == 3
    assert lib.tts_lstm_create(32, 48, 1, None) == 1
    assert lib.tts_lstm_create(32, 48, 1, ctypes.byref(h)) == 0
    assert lib.tts_lstm_reserve_floats(h, 2, 3) == 2 * 3 * 2 * 48 * 5 + 2 * 2 * 48
    assert lib.tts_lstm_reserve_floats(h, 0, 3) == 0
    lens = n.i32_array([3, 1])
    assert lib.tts_lstm_forward(h, None, lens, 2, 3, None, None, None, None, None, None, None) == 1
    assert lib.tts_lstm_forward(h, ctypes.c_void_p(16), lens, 2, 3, None, None, ctypes.c_void_p(16), None, None, None,
                                None) == 1  # weights not set
    assert lib.tts_lstm_set_weights(h, None, None, None, None, None) == 1
    lib.tts_lstm_destroy(h)
