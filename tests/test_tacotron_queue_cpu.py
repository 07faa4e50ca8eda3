"""Tacotron / TacotronGST decoder memory queue (memory_size > r, layers/tacotron.py:279-287, 310,
396-404), the parts that need no GPU: constructor shapes, the weight spec, and both CPU oracles
against the reference's own queue runs (tests/golden/tmq_*.npz, made by
tests/golden/make_golden_tacotron_queue.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, golden_flags, load_pkg, rel_rms, weights_mod

TMQ_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "tmq_*.npz")))


def test_queue_fixtures_present():
    assert len(TMQ_CASES) == 7
    for c in TMQ_CASES:
        z = golden(c)
        fl = golden_flags(z)
        assert fl["memory_size"] > fl["r"]
        assert z["align"].shape[0] >= 2, "a run of one step never reads a shifted queue"


def test_constructor_queue_shapes():
    t = load_pkg("tacotron")
    m = t.Tacotron(130, 0, r=2, memory_size=5)
    sd = m.state_dict()
    assert tuple(sd["decoder.prenet.layers.0.linear_layer.weight"].shape) == (256, 400)
    assert tuple(sd["decoder.memory_init.weight"].shape) == (1, 400)
    assert tuple(sd["decoder.proj_to_mel.weight"].shape) == (160, 256)
    assert tuple(sd["decoder.stopnet.linear.weight"].shape) == (1, 256 + 160)
    w = weights_mod().tacotron_gst_weights(1, num_chars=130, r=2, memory_size=5, gst=False, location_attn=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    np.testing.assert_array_equal(m.state_dict()["decoder.memory_init.weight"].numpy(),
                                  w["decoder.memory_init.weight"])


def test_constructor_memory_size_zero_means_r():
    t = load_pkg("tacotron")
    m = t.TacotronGST(130, 0, r=3, memory_size=0)
    assert m.memory_size == 3
    sd = m.state_dict()
    assert tuple(sd["decoder.prenet.layers.0.linear_layer.weight"].shape) == (256, 240)
    assert tuple(sd["decoder.memory_init.weight"].shape) == (1, 240)


def test_constructor_short_queue_raises():
    t = load_pkg("tacotron")
    with pytest.raises(ValueError):
        t.Tacotron(130, 0, r=5, memory_size=3)


def test_setup_model_builds_queue_checkpoint_shapes():
    """A config with r < memory_size (every shipped Tacotron config has memory_size 5, "useful if r < 5")."""
    gu = load_pkg("generic_utils")
    c = gu.default_config("config_tacotron_gst.json")
    c.r = 2
    m = gu.setup_model(130, 0, c)
    assert (m.r, m.memory_size) == (2, c.memory_size) and c.memory_size == 5
    assert tuple(m.state_dict()["decoder.prenet.layers.0.linear_layer.weight"].shape) == (256, 400)


def test_spec_memory_size_zero():
    w = weights_mod()
    shapes = {k: s for k, s, _ in w.tacotron_gst_spec(r=2, memory_size=0)}
    assert shapes["decoder.memory_init.weight"] == (1, 160)
    assert shapes["decoder.prenet.layers.0.linear_layer.weight"] == (256, 160)
    sd = w.tacotron_gst_weights(0, r=2, memory_size=0)
    assert np.isfinite(sd["decoder.prenet.layers.0.linear_layer.weight"]).all()


def _oracle_weights(fl):
    return weights_mod().tacotron_gst_weights(0, num_speakers=fl["num_speakers"], r=fl["r"],
                                              memory_size=fl["memory_size"], location_attn=fl["location_attn"],
                                              trans_agent=fl["trans_agent"], gst=fl["model"] == "TacotronGST",
                                              prenet_bn=fl.get("prenet_type", "original") == "bn")


@pytest.mark.parametrize("case", TMQ_CASES)
def test_numpy_oracle_matches_queue_fixture(case):
    """tests/test_oracle_golden.py's Tacotron check pointed at the queue fixtures."""
    from oracle.tacotron_oracle import TacotronOracle
    z = golden(case)
    fl = golden_flags(z)
    o = TacotronOracle(_oracle_weights(fl), dtype=np.float64, **{k: v for k, v in fl.items() if k != "prenet_type"})
    sid = int(z["speaker_id"])
    enc = o.encoder(z["ids"], None if sid < 0 else sid, z["style_mel"] if "style_mel" in z else None)
    assert rel_rms(enc, z["enc"]) < 1e-5
    mel, stop, align = o.decoder(z["enc"])
    assert mel.shape == z["mel"].shape, "frame count differs from the reference"
    np.testing.assert_array_equal(align.argmax(1), z["align"].argmax(1))
    assert rel_rms(mel, z["mel"]) < 1e-5
    assert np.abs(align - z["align"]).max() < 1e-5
    assert np.abs(stop - z["stop"]).max() < 1e-5
    if "linear" in z:
        assert rel_rms(o.postnet(z["mel"]), z["linear"]) < 1e-5


@pytest.mark.parametrize("case", TMQ_CASES)
def test_torch_oracle_matches_queue_fixture(case):
    from oracle.tacotron_torch import TacotronTorchCPU
    z = golden(case)
    fl = golden_flags(z)
    sid = int(z["speaker_id"])
    res = TacotronTorchCPU(_oracle_weights(fl), **fl).inference(
        z["ids"], None if sid < 0 else sid, z["style_mel"] if "style_mel" in z else None)
    assert res["mel"].shape == z["mel"].shape, "frame count differs from the reference"
    np.testing.assert_array_equal(res["align"].argmax(1), z["align"].argmax(1))
    assert rel_rms(res["mel"], z["mel"]) < 1e-5
    assert np.abs(res["align"] - z["align"]).max() < 1e-5
    assert np.abs(res["stop"] - z["stop"]).max() < 1e-5
