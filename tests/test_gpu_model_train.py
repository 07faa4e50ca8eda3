"""The composed Tacotron2 with every trainable layer on the device (layers.LSTM, layers.ConvBNBlock and
layers.Decoder swapped into model_train_util's model): one training iteration by hand on every case of
model_train_util.py, the four outputs, the losses, the two gradient norms and EVERY parameter gradient within the
relative bound of the float64 twin and of the reference's float64 run (tests/golden/model_train.npz); then two
iterations through train.train_batch itself with the masks the device layers drew replayed in the twin; then
run-to-run determinism.  What the per-layer tests cannot see is covered here: the two upstream gradients of the
decoder outputs through transposed views, the encoder output's gradient through pad_packed_sequence into the LSTM,
the chained grad_x of the conv-BN blocks, and the separate stopnet's backward after the main optimizer's step.

Measured on an MI355X (tools/model_train_report.py; profiles/model_train.json, "device_errors"): every figure is
inside its bound.  The nearest to its bound is grad_decoder.go_frame_init.weight of "ref", 4.4e-6 against 5.4e-6; the
largest is grad_encoder.lstm.weight_ih_l0 of "joint", 7.8e-6 against 1.1e-5 (the reference's own float32 run is at
2.7e-6 there); "small" stays at or below 1.1e-6 against 4e-6.
"""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import model_train_util as mu  # noqa: E402
import train_util as tu  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "model_train.npz"))
STOPNET = ("grad_decoder.stopnet.1.linear_layer.weight", "grad_decoder.stopnet.1.linear_layer.bias")


def load_pkg(name):
    return importlib.import_module("your-voice-tts_amd." + name)


def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def device(case):
    """One iteration by hand on the device, computed once and shared; do not modify."""
    return mu.device_iterate(case, load_pkg("layers"), load_pkg("losses"))


@pytest.mark.parametrize("case", list(mu.CASES))
def test_iteration_by_hand_within_the_bound(case):
    got, want = device(case), mu.twin(case)
    mu.compare(case, got, want, GOLD)
    lens = np.asarray(mu.CASES[case]["text_lens"])
    padded = np.arange(lens.max())[None, :] >= lens[:, None]  # [B, L]
    assert padded.any()
    for name, rows in (("alignments", lambda a: a.transpose(0, 2, 1)[padded]), ("grad_encoder_outputs", lambda a: a[padded])):
        assert not rows(want[name]).any(), name  # the reference's are zero there
        assert not rows(got[name]).any(), f"{name} is not zero on the padded rows"


def _tol(case, name):
    return mu.tolerance(GOLD[mu.key(case, name, "ref32")])


@pytest.mark.parametrize("case", ["ref", "joint"])
def test_train_batch_is_the_twin_s_iteration(case):
    layers, optim, train = load_pkg("layers"), load_pkg("optim"), load_pkg("train")
    c, inp = mu.CASES[case], mu.inputs(case)
    cfg = tu.config(separate_stopnet=c["sep"], r=c["r"], loss_masking=c["masked"])
    model = mu.device_model(case, layers, inp["weights"])
    dec = model.decoder
    opt = optim.Adam(model.parameters(), lr=cfg.lr, weight_decay=0)
    opt_st = optim.Adam(dec.stopnet.parameters(), lr=cfg.lr, weight_decay=0) if c["sep"] else None
    twin = mu.Twin(case, inp["weights"])
    batch = mu.batch(inp, "cuda")
    for it in range(2):
        if it:  # from the device's parameters and buffers: Adam's sensitivity near zero gradients stays out of it
            twin.load(model.state_dict())
        torch.manual_seed(700 + it)
        out = train.train_batch(model, cfg, batch, opt, opt_st)
        want = twin.run(inp, masks=mu.device_masks(model))
        what = f"train_batch {case} iteration {it}"
        for name, t in zip(mu.OUTPUTS, out["outputs"]):
            mu.check(t.detach().cpu().numpy(), want[name], f"{what} {name}", _tol(case, name))
        for name in mu.SCALARS:  # grad_norm: before the clip, over all parameters
            mu.check(mu.scalar(out[name]), mu.scalar(want[name]), f"{what} {name}", _tol(case, name))
        assert np.array_equal(out["stop_targets"].cpu().numpy(), inp["stop_targets"])
        if c["sep"]:  # check_update(model.decoder.stopnet, 1.0) clipped these in place
            clip = min(1.0, 1.0 / (want["grad_norm_st"] + 1e-6))
            for name, p in zip(STOPNET, dec.stopnet.parameters()):
                mu.check(p.grad.cpu().numpy(), want[name] * clip, f"{what} clipped {name}", _tol(case, name))
        state = model.state_dict()
        for k, v in want["buffers"].items():
            if k.endswith("num_batches_tracked"):
                assert int(state[k]) == int(v) == it + 1, k
            else:
                mu.check(state[k].cpu().numpy(), v, f"{what} {k}")
    assert dec.repacks == 2


def test_deterministic():
    """Two runs from the same state: the same bits on every tensor but the embedding's gradient, which is torch's own
    scatter-add (atomics in an order that varies) and not a kernel of this package."""
    a, b = device("ref"), mu.device_iterate("ref", load_pkg("layers"), load_pkg("losses"))
    for name in mu.tensor_names("ref"):
        if name != "grad_embedding.weight":
            assert bitwise(a[name], b[name]), name
    for name in mu.SCALARS[:3]:
        assert a[name] == b[name], name
