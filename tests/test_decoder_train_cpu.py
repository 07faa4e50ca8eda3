"""The trainable decoder without a GPU: the float64 restatement of decoder_train_util.py against the reference's own
float64 run (tests/golden/decoder_train.npz) on every case of the fixture, seven mutants of the restatement (the six
of the design and one that delays the decoder cell's context in the forward) that must each break the bound on a
named case, and the module's contract (state dict, unsupported options, the "no GPU" error, the six symbols)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import decoder_train_util as du  # noqa: E402

layers = importlib.import_module("your-voice-tts_amd.layers")
native = importlib.import_module("your-voice-tts_amd._native")
GOLD = np.load(os.path.join(HERE, "golden", "decoder_train.npz"))

CPU_CASES = list(du.FIXTURE_CASES)  # every case of the fixture ("chunks", the largest, restates in a few seconds)


def test_chunks_case_passes_one_reduction_chunk_and_is_no_multiple_of_it():
    c = du.CASES["chunks"]
    rows = len(c["lens"]) * c["T"]
    assert rows > du.KC and rows % du.KC


def test_kept_prenet_preactivations_are_off_the_kink():
    for case in ("t6", "nodrop"):
        assert du.min_kept_preactivation(du.inputs(case)) >= du.MIN_Z


@pytest.mark.parametrize("case", CPU_CASES)
def test_restatement_matches_the_reference_in_float64(case):
    r = du.restated(case)
    for name in du.tensor_names(case):
        ref64 = GOLD[du.key(case, name, 64)]
        v = du.ratio(du.stored(case, name, r[name]), ref64, du.scale_of(case, name, r))
        # the reference keeps alpha's initial 1e-7 and u = 0.5 in float32 even in its float64 run: 1e-8 of slack
        assert v <= 1e-7, f"{case} {name}: {v:.3e}"


def test_fixture_holds_the_reference_float32_figure_inside_the_bound():
    for case in du.FIXTURE_CASES:
        for name in du.tensor_names(case):
            own = float(GOLD[du.key(case, name, "ref32")])
            assert own <= du.TOL, (case, name, own)  # so the tolerance is 4e-6 on every tensor of these cases
            assert du.tolerance({case: {name: own}}, case, name) == max(du.TOL, 4 * own)


MUTANTS = [("cell_not_carried", "t6"), ("no_shift", "t6"), ("mask_joins", "t6"), ("att_ctx_t", "t6"),
           ("stop_attached", "t6"), ("zero_go", "t6"), ("dec_ctx_prev", "t6")]


@pytest.mark.parametrize("mutant,case", MUTANTS)
def test_mutant_breaks_the_bound(mutant, case):
    good, bad = du.restated(case), du.restate(du.inputs(case), mutant=mutant)
    worst = max(du.ratio(bad[n], good[n], du.scale_of(case, n, good)) for n in du.tensor_names(case))
    print(f"{mutant} on {case}: {worst:.3e}")
    assert worst > du.TOL


def _decoder(**kw):
    args = dict(in_features=512, inputs_dim=80, r=1, attn_win=False, attn_norm="sigmoid", prenet_type="original",
                prenet_dropout=True, forward_attn=True, trans_agent=False, forward_attn_mask=False, location_attn=False,
                separate_stopnet=True)
    args.update(kw)
    return layers.Decoder(**args)


def test_state_dict_is_the_reference_decoder_s():
    sd = _decoder().state_dict()
    assert list(sd) == [str(k) for k in GOLD["state_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in GOLD["state_shapes"]]
    assert tuple(native.DECTRAIN_PARAMS) == du.PARAMS and set(du.PARAMS) == set(sd)
    t = du.torch_decoder("t6")
    t.load_state_dict(sd)
    _decoder().load_state_dict(t.state_dict())


@pytest.mark.parametrize("kw,word", [(dict(location_attn=True), "location_attn"), (dict(trans_agent=True), "trans_agent"),
                                     (dict(prenet_type="bn"), "prenet_type")])
def test_unsupported_options_raise(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _decoder(**kw)

    class Model(torch.nn.Module):
        pass

    model = Model()
    model.decoder = old = du.torch_decoder("small")
    if "location_attn" in kw:
        old.attention_layer.location_attention = True
    elif "trans_agent" in kw:
        old.attention_layer.trans_agent = True
    else:
        old.prenet.prenet_type = "bn"
    with pytest.raises(NotImplementedError, match=word):
        layers.use_device_decoder(model)
    assert model.decoder is old  # raised before it touched the model


def test_inference_and_eval_only_options_raise():
    d = _decoder(attn_win=True, forward_attn_mask=True)  # accepted
    for name in ("inference", "inference_truncated", "inference_step"):
        with pytest.raises(NotImplementedError, match="Tacotron2.inference"):
            getattr(d, name)(torch.zeros(1, 3, 512))
    d.eval()
    with pytest.raises(NotImplementedError, match="eval"):
        d(torch.zeros(1, 3, 512), torch.zeros(1, 2, 80), None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-GPU error needs a machine without one")
def test_forward_without_a_gpu_raises_the_package_error():
    with pytest.raises(RuntimeError, match="no GPU"):
        _decoder()(torch.zeros(1, 3, 512), torch.zeros(1, 2, 80), None)


def test_native_declares_the_six_symbols():
    names = ["tts_dectrain_" + s for s in ("create", "destroy", "set_weights", "reserve_floats", "forward", "backward")]
    assert all(n in native.EXPORTS for n in names)
    lib = native.load_library()
    for n in names:
        assert getattr(lib, n).argtypes is not None
    assert lib.tts_dectrain_reserve_floats.restype is native.ctypes.c_int64
