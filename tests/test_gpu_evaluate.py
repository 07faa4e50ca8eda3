"""evaluate.evaluate_batch / evaluate on the collated fixture batch: the three losses equal eval_util.py's
float64 restatement applied to the same forward's outputs copied to the host, at the fp64 bound of
eval_util.py; the switches of train.py:327-339 (loss_masking, stopnet); the per-r stop-target grouping
against the fixture (case f).  The forward itself is pinned by the tf_* / ttf_* tests, not here."""
import ast
import functools

import numpy as np
import pytest
import torch

import eval_util as eu
from conftest import golden, load_pkg, weights_mod

pytestmark = pytest.mark.gpu
Z = golden("eval")
MODELS = {"tacotron2_r1": ("config_tacotron2.json", 1), "tacotron2_r2": ("config_tacotron2.json", 2),
          "tacotron_gst_r5": ("config_tacotron_gst.json", 5)}


@functools.lru_cache(maxsize=None)
def _ap():
    return load_pkg("audio").AudioProcessor(**ast.literal_eval(str(Z["audio"])))


@functools.lru_cache(maxsize=None)
def _items():
    items = eu.collate_items(golden("audio_example1")["pcm"])
    for i, d in enumerate(items):  # ids of the test weight generator, at the fixture's text lengths
        d["text"] = weights_mod().synthetic_ids(len(d["text"]), 900 + i).astype(np.int32)
    return items


@functools.lru_cache(maxsize=None)
def _run(case):
    """One model, the collated fixture batch and its evaluate_batch result, shared by the tests."""
    gu = load_pkg("generic_utils")
    name, r = MODELS[case]
    c = gu.default_config(name)
    c.r = r
    model = gu.setup_model(130, c).cuda().eval()
    batch = load_pkg("datasets").collate_fn(_items(), _ap(), r)
    return dict(c=c, r=r, model=model, batch=batch, out=load_pkg("evaluate").evaluate_batch(model, c, batch))


@pytest.fixture(params=sorted(MODELS))
def run(request):
    return _run(request.param)


def _expected(run, out, masked=True):
    """The restated losses on the forward's outputs copied to the host: {name: (value, terms, per sentence)}."""
    c, batch = run["c"], run["batch"]
    linear, mel, mel_lengths = batch[3].cpu(), batch[4].cpu(), batch[5].tolist()
    dec, post, _, stop = (t.cpu() for t in out["outputs"])
    tacotron = c.model != "Tacotron2"
    kind = "l1" if tacotron else "mse"
    lengths = mel_lengths if masked else None
    bce, n = eu.bce_with_logits(stop, out["stop_targets"].cpu())
    return dict(decoder_loss=eu.elementwise_loss(kind, dec, mel, lengths),
                postnet_loss=eu.elementwise_loss(kind, post, linear if tacotron else mel, lengths),
                stop_loss=(bce, n, None))


def _check(run, out, masked=True, stopnet=True):
    want = _expected(run, out, masked)
    for k in ("decoder_loss", "postnet_loss") + (("stop_loss",) if stopnet else ()):
        ref, n, _ = want[k]
        print(f"{run['c'].model} r={run['r']} {k}: {out[k]!r} vs {ref!r} ({n} terms)")
        assert isinstance(out[k], float) and np.isfinite(out[k]) and out[k] > 0
        assert eu.within(out[k], ref, n), k
    assert out["loss"] == out["decoder_loss"] + out["postnet_loss"] + out["stop_loss"]
    return want


def test_gpu_evaluate_batch(run):
    out, batch, r = run["out"], run["batch"], run["r"]
    tpad = batch[4].shape[1]
    dec, post, align, stop = out["outputs"]
    width = 1025 if run["c"].model != "Tacotron2" else 80
    assert dec.shape == (4, tpad, 80) and post.shape == (4, tpad, width) and stop.shape == (4, tpad // r)
    want = _check(run, out)
    shape = {"decoder": dec.shape, "postnet": post.shape}
    for k in ("decoder", "postnet"):
        per = out["per_sentence"][k]
        assert per.shape == (4,) and per.dtype == torch.float64 and per.is_cuda
        for b in range(4):
            assert eu.within(float(per[b]), want[k + "_loss"][2][b], eu.sentence_terms(shape[k], batch[5].tolist(), b))


def test_gpu_grouped_stop_targets(run):
    got = run["out"]["stop_targets"]
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), Z[f"stop_grouped_r{run['r']}"])


def test_gpu_evaluate_batch_switches(run):
    ev = load_pkg("evaluate")
    c = type(run["c"])(run["c"])
    c.loss_masking = False
    c.stopnet = False
    out = ev.evaluate_batch(run["model"], c, run["batch"])
    for a, b in zip(out["outputs"], run["out"]["outputs"]):
        assert torch.equal(a, b)
    _check(run, out, masked=False, stopnet=False)
    assert out["stop_loss"] == 0
    assert out["decoder_loss"] != run["out"]["decoder_loss"]  # (the padding rows count now)


def test_gpu_evaluate_loop():
    run, ap, items = _run("tacotron2_r1"), _ap(), _items()
    ev, ds = load_pkg("evaluate"), load_pkg("datasets")
    got = ev.evaluate(run["model"], run["c"], ap, items, 3)
    parts = [ev.evaluate_batch(run["model"], run["c"], ds.collate_fn(chunk, ap, 1)) for chunk in (items[:3], items[3:])]
    assert sorted(got) == ["loss_decoder", "loss_postnet", "stop_loss"]
    for k, src in (("loss_decoder", "decoder_loss"), ("loss_postnet", "postnet_loss"), ("stop_loss", "stop_loss")):
        assert got[k] == (parts[0][src] + parts[1][src]) / 2
