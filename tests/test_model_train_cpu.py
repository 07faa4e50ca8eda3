"""The composed Tacotron2 of the training path without a GPU: the float64 twin of model_train_util.py against the
reference's own float64 run (tests/golden/model_train.npz) on every case of the fixture, five mutants of the twin
that must each break the relative bound on a named tensor ("query_99" passes the old max(1, .) form: the reason for
the relative one), the float32 torch model inside the bound (the reference alone satisfies it), and the builder's
state dict before and after the three swaps."""
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import decoder_train_util as du  # noqa: E402
import model_train_util as mu  # noqa: E402

layers = importlib.import_module("your-voice-tts_amd.layers")
GOLD_PATH = os.path.join(HERE, "golden", "model_train.npz")
GOLD = np.load(GOLD_PATH)


def test_cases_are_the_design_s_and_off_the_kink():
    assert os.path.getsize(GOLD_PATH) < 1 << 20
    assert mu.CASES["b17"]["text_lens"] == list(range(17, 0, -1)) and len(set(mu.CASES["b17"]["mel_lens"])) > 1
    assert mu.CASES["l70"]["text_lens"] == [70, 33, 1] and mu.CASES["l70"]["frames"] // mu.CASES["l70"]["r"] == 4
    assert mu.CASES["small"]["dims"]["E"] == du.MODEL["E"] and mu.CASES["small"]["dims"]["mel"] == du.MODEL["mel"]
    for case in mu.CASES:  # (inputs() itself asserts that the search ends within its cap)
        inp = mu.inputs(case)
        assert inp["attempt"] < mu.ATTEMPTS and mu.min_kept_preactivation(inp) >= mu.MIN_Z, case
        assert inp["text_lens"] == sorted(inp["text_lens"], reverse=True)


@pytest.mark.parametrize("case", mu.FIXTURE_CASES)
def test_twin_matches_the_reference_in_float64(case):
    r = mu.twin(case)
    # the reference keeps forward attention's initial 1e-7 in float32 even in its float64 run (1.2e-8 of it); without
    # forward attention the two are the same arithmetic
    slack = 1e-7 if mu.CASES[case]["fwd"] else 1e-12
    for name in mu.tensor_names(case):
        v = mu.ratio(mu.stored(case, name, r[name]), GOLD[mu.key(case, name, 64)], mu.scale_of(case, name, r))
        assert v <= slack, f"{case} {name}: {v:.3e}"
    for name in mu.SCALARS:
        assert mu.ratio(r[name], GOLD[mu.key(case, name, 64)]) <= slack, (case, name)


def test_profile_holds_the_twin_s_figure_at_rounding_level():
    import json
    doc = json.load(open(os.path.join(os.path.dirname(HERE), "profiles", "model_train.json")))["reference_fp32"]
    for case, figures in doc["twin_against_reference_fp64"].items():
        assert max(figures.values()) <= (1e-7 if mu.CASES[case]["fwd"] else 1e-12), case
    for case in mu.FIXTURE_CASES:
        for name in mu.tensor_names(case) + list(mu.SCALARS):
            assert doc["per_case"][case][name] == float(GOLD[mu.key(case, name, "ref32")]), (case, name)


@pytest.mark.parametrize("case", list(mu.CASES))
def test_float32_torch_model_is_within_the_bound(case):
    mu.compare(case, mu.torch32(case), mu.twin(case), GOLD, what="torch float32")


MUTANTS = [("no_residual", "small", "postnet_output"),
           ("stop_leaks", "small", "grad_decoder.linear_projection.linear_layer.weight"),
           ("one_upstream", "small", "grad_decoder.linear_projection.linear_layer.weight"),
           ("padded_rows", "small", "grad_encoder.lstm.weight_hh_l0"),
           ("query_99", "small", mu.QUERY),
           ("padded_rows", "ref", "grad_encoder.lstm.weight_hh_l0"),
           ("query_99", "ref", mu.QUERY)]


@pytest.mark.parametrize("mutant,case,name", MUTANTS)
def test_mutant_breaks_the_bound(mutant, case, name):
    good, bad = mu.twin(case), mu.twin(case, mutant)
    tol = mu.tolerance(GOLD[mu.key(case, name, "ref32")]) if case in mu.FIXTURE_CASES else mu.TOL
    v = mu.ratio(bad[name], good[name], mu.scale_of(case, name, good))
    broken = [n for n in mu.tensor_names(case) if mu.ratio(bad[n], good[n], mu.scale_of(case, n, good)) > mu.TOL]
    print(f"{mutant} on {case}: {name} {v:.3e} (bound {tol:.1e}); {len(broken)} tensors differ")
    assert v > tol


@pytest.mark.parametrize("case", ["ref"])
def test_query_99_passes_the_old_form_of_the_bound(case):
    """max |got - ref64| <= 4e-6 * max(1, max |ref64|) is an absolute 4e-6 against a gradient this small (2.7e-4 at
    the reference's dimensions; at "small"'s the gradient is ten times larger and the old form would notice)."""
    good, bad = mu.twin(case)[mu.QUERY], mu.twin(case, "query_99")[mu.QUERY]
    old, new = du.ratio(bad, good), mu.ratio(bad, good)
    print(f"{case}: max|grad| {np.abs(good).max():.3e}, old form {old:.3e}, relative form {new:.3e}")
    assert old <= du.TOL < new and abs(new - 0.01) < 1e-9


def _keys_and_shapes(sd):
    return list(sd), [",".join(str(d) for d in v.shape) for v in sd.values()]


@pytest.mark.parametrize("r", [1, 2])
def test_builder_has_the_reference_state_dict_and_the_swaps_keep_it(r):
    want = [str(k) for k in GOLD[f"state_keys_r{r}"]], [str(s) for s in GOLD[f"state_shapes_r{r}"]]
    m = mu.build_model(mu.REF, r=r)
    assert _keys_and_shapes(m.state_dict()) == want
    spec = mu.state_shapes(mu.REF, r)
    assert (list(spec), [",".join(str(d) for d in s) for s in spec.values()]) == want
    layers.use_device_decoder(layers.use_device_convs(layers.use_device_lstm(m)))
    assert isinstance(m.decoder, layers.Decoder) and isinstance(m.encoder.lstm, layers.LSTM)
    assert all(isinstance(b, layers.ConvBNBlock) for b in list(m.encoder.convolutions) + list(m.postnet.convolutions))
    assert _keys_and_shapes(m.state_dict()) == want


def test_swaps_keep_the_small_model_s_values():
    import torch
    m = mu.model_for("small", mu.inputs("small")["weights"])
    before = {k: v.clone() for k, v in m.state_dict().items()}
    layers.use_device_decoder(layers.use_device_convs(layers.use_device_lstm(m)))
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
