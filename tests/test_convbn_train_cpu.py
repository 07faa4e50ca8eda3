"""CPU: the float64 restatement of tests/convbn_train_util.py against the convbn_train.npz fixture (the reference's
ConvBNBlock, Encoder.convolutions and Postnet.convolutions with autograd, float32 and float64, the dropout masks of
the reference run), the two conditions that make the GPU test's bound meetable, six mutants that show the
comparison can fail, and the surface of layers.ConvBNBlock / layers.use_device_convs that needs no GPU."""
import numpy as np
import pytest
import torch
from torch import nn

import convbn_train_util as cu
import encoder_util as eu
from conftest import golden, load_pkg


@pytest.fixture(scope="module")
def fixture():
    return golden("convbn_train")


@pytest.fixture(scope="module")
def restated(fixture):
    return {case: cu.restate(cu.inputs(case), cu.masks(fixture, case)) for case in cu.CASES}


def test_bound_is_the_projects():
    assert cu.TOL == eu.ALIGN_ATOL == 4e-6


def test_chunk_case_crosses_two_chunks_and_ends_partial():
    n = cu.CASES["chunks"]["B"] * cu.CASES["chunks"]["T"]
    assert n // cu.KC == 2 and n % cu.KC
    src = open(load_pkg("_native")._HERE + "/csrc/convbn_train.hip").read()
    assert f"constexpr int CB_KC = {cu.KC};" in src


@pytest.mark.parametrize("case", list(cu.CASES))
def test_restatement_lies_within_the_bound_of_the_reference_float64(case, fixture, restated):
    for name in cu.tensor_names(case):
        cu.check(cu.stored(case, name, restated[case][name]), fixture[cu.key(case, name, 64)], f"{case} {name}",
                 cu.bias_scale(name, restated[case]))


@pytest.mark.parametrize("case", list(cu.CASES))
def test_reference_float32_lies_within_the_bound(case, fixture, restated):
    for name in cu.tensor_names(case):
        scale = cu.bias_scale(name, restated[case])
        cu.check(fixture[cu.key(case, name, 32)], fixture[cu.key(case, name, 64)], f"{case} {name} (fixture)", scale)
        cu.check(fixture[cu.key(case, name, 32)], cu.stored(case, name, restated[case][name]), f"{case} {name}", scale)
    steps = fixture[cu.key(case, "num_batches_tracked", "i")]
    assert steps.tolist() == [2] * len(cu.CASES[case]["blocks"])


@pytest.mark.parametrize("case", list(cu.CASES))
def test_input_conditions(case, restated):
    """n >= 6, and no kept element of a relu block within 1e-5 of the kink in float64."""
    r = restated[case]
    print(f"{case}: n = {r['n']}, min |z64| over kept relu elements = {r['minz']:.3e}")
    assert r["n"] >= cu.MIN_N
    assert r["minz"] >= cu.MIN_Z


def test_masks_are_dropout_masks(fixture):
    for case in cu.CASES:
        for i, m in enumerate(cu.masks(fixture, case)):
            assert set(np.unique(m)) <= {0, 1} and 0 < m.mean() < 1, (case, i)


MUTANT_TENSORS = {"unbiased_norm": "out", "biased_running": "rv1_0", "no_xhat_term": "grad_x", "no_flip": "grad_x",
                  "edge_pad": "out", "scale1": "out"}


@pytest.mark.parametrize("mutant", cu.MUTANTS)
def test_mutants_leave_the_bound(mutant, fixture, restated):
    """Each deliberate error is at least 100x outside the bound on the tensor it is aimed at."""
    case = "small"
    bad = cu.restate(cu.inputs(case), cu.masks(fixture, case), mutant=mutant)
    name = MUTANT_TENSORS[mutant]
    v = cu.ratio(bad[name], restated[case][name])
    print(f"{mutant}: {name} ratio {v:.3e}")
    assert v >= 100 * cu.TOL
    with pytest.raises(AssertionError):
        cu.check(cu.stored(case, name, bad[name]), fixture[cu.key(case, name, 64)], f"{mutant} {name}")


def test_eval_restatement_matches_torch():
    """block_forward(training=False) is torch's eval(): running statistics, no dropout, nothing moves."""
    inp = cu.inputs("small")
    blk = inp["blocks"][0]
    g = np.random.Generator(np.random.PCG64(5))
    rm, rv = g.standard_normal(32), g.uniform(0.5, 2.0, 32)
    net = nn.Sequential(nn.Conv1d(48, 32, 5, padding=2), nn.BatchNorm1d(32), nn.Tanh(), nn.Dropout(0.5)).double()
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in cu.state_dict(blk).items()}
    sd["net.1.running_mean"], sd["net.1.running_var"] = torch.from_numpy(rm), torch.from_numpy(rv)
    net.load_state_dict({k[len("net."):]: v for k, v in sd.items()})
    want = net.eval()(torch.from_numpy(inp["x"]).double()).detach().numpy()
    got, _, rm2, rv2 = cu.block_forward(inp["x"].astype(np.float64), blk, None, rm, rv, training=False)
    assert cu.ratio(got, want) <= 1e-12 and rm2 is rm and rv2 is rv


# ------------------------------------------------------------------ module surface
def test_state_dict_is_the_reference_blocks(fixture):
    layers = load_pkg("layers")
    m = layers.ConvBNBlock(512, 512, 5, "relu")
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in fixture["state_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in fixture["state_shapes"]]
    assert [type(t).__name__ for t in m.net] == ["Conv1d", "BatchNorm1d", "ReLU", "Dropout"]
    assert [type(t).__name__ for t in layers.ConvBNBlock(80, 512, 5, "tanh").net][2] == "Tanh"
    assert len(layers.ConvBNBlock(512, 80, 5).net) == 3
    assert m.net[0].padding == (2,) and m.net[-1].p == 0.5


def test_reference_shaped_state_dict_loads_both_ways():
    layers = load_pkg("layers")
    blk = cu.inputs("small")["blocks"][0]
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cu.state_dict(blk).items()}
    ours = layers.ConvBNBlock(48, 32, 5, "tanh")
    ours.load_state_dict(sd)
    assert all(torch.equal(ours.state_dict()[k], sd[k]) for k in sd)
    theirs = cu.tiny_model().encoder.convolutions[0].__class__(48, 32, "tanh")
    theirs.load_state_dict(ours.state_dict())
    assert all(torch.equal(theirs.state_dict()[k], sd[k]) for k in sd)


def test_use_device_convs_swaps_every_block_and_is_idempotent():
    layers = load_pkg("layers")
    model = cu.tiny_model()
    model.postnet.convolutions[1].eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert layers.use_device_convs(model) is model
    blocks = list(model.encoder.convolutions) + list(model.postnet.convolutions)
    assert len(blocks) == 5 and all(isinstance(b, layers.ConvBNBlock) for b in blocks)
    assert [b.nonlinear for b in blocks] == ["relu", "relu", "tanh", "tanh", None]
    assert [b.training for b in blocks] == [True, True, True, False, True]
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert layers.use_device_convs(model) is model
    assert all(a is b for a, b in zip(blocks, list(model.encoder.convolutions) + list(model.postnet.convolutions)))
    only_encoder = nn.Module()
    only_encoder.encoder = cu.tiny_model().encoder
    layers.use_device_convs(only_encoder)
    assert all(isinstance(b, layers.ConvBNBlock) for b in only_encoder.encoder.convolutions)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_cpu_tensor_raises_no_gpu():
    layers = load_pkg("layers")
    m = layers.ConvBNBlock(48, 32, 5, "tanh")
    with pytest.raises(RuntimeError, match="no GPU"):
        m(torch.zeros(2, 48, 3))
    with pytest.raises(RuntimeError, match="no GPU"):
        m.eval()(torch.zeros(2, 48, 3))


@pytest.mark.parametrize("kw", [dict(kernel_size=3), dict(in_channels=20), dict(out_channels=40),
                                dict(nonlinear="sigmoid")])
def test_unsupported_constructions_raise(kw):
    layers = load_pkg("layers")
    args = dict(in_channels=48, out_channels=32, kernel_size=5, nonlinear="relu")
    args.update(kw)
    with pytest.raises(NotImplementedError):
        layers.ConvBNBlock(**args)


def test_unsupported_norm_settings_raise():
    layers = load_pkg("layers")
    for change in (lambda n: setattr(n, "momentum", None), lambda n: setattr(n, "track_running_stats", False)):
        m = layers.ConvBNBlock(48, 32, 5, "tanh")
        change(m.net[1])
        with pytest.raises(NotImplementedError):
            m(torch.zeros(2, 48, 3))


def test_c_abi_rejects_before_any_launch():
    """UNSUPPORTED constructions at create; INVALID (null pointers, weights not set) from the calls: none touches
    the GPU."""
    import ctypes
    n = load_pkg("_native")
    lib = n.load_library()
    h = ctypes.c_void_p()
    assert lib.tts_convbn_create(48, 32, 3, 1, ctypes.byref(h)) == 3
    assert lib.tts_convbn_create(20, 32, 5, 1, ctypes.byref(h)) == 3
    assert lib.tts_convbn_create(48, 40, 5, 1, ctypes.byref(h)) == 3
    assert lib.tts_convbn_create(48, 32, 5, 3, ctypes.byref(h)) == 1
    assert lib.tts_convbn_create(48, 32, 5, 1, None) == 1
    assert lib.tts_convbn_create(48, 32, 5, 1, ctypes.byref(h)) == 0
    assert lib.tts_convbn_reserve_floats(h, 2, 3) == 2 * 32 * 3 + 2 * 32 + 1
    assert lib.tts_convbn_reserve_floats(h, 0, 3) == 0
    p = ctypes.c_void_p(16)
    assert lib.tts_convbn_forward(h, p, 2, 3, p, 2.0, p, p, 0.1, 1e-5, 1, p, None, None) == 1  # weights not set
    assert lib.tts_convbn_backward(h, p, 2, 3, p, p, p, p, None, None, None, None, None) == 1
    assert lib.tts_convbn_set_weights(h, None, None, None, None, None) == 1
    lib.tts_convbn_destroy(h)
