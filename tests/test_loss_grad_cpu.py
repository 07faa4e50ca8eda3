"""CPU: the float64 restatement of the criteria's gradients (loss_grad_util.py) against the reference's own
gradients (loss_grad.npz, tests/golden/make_golden_loss_grad.py); the GPU test's two bounds, passed by the
restatement rounded to float32 (so that a miss on the device is the kernel's); the sequencing of
``train.train_batch`` on a CPU stand-in with the criteria and the update replaced by torch's; and that the
torch-only iteration lowers the loss on the fixed batch of train_util.py, which the GPU test then asks of
``train_batch``.
"""
import numpy as np
import pytest
import torch

import eval_util as eu
import loss_grad_util as lg
import train_util as tu
from conftest import golden, load_pkg

Z = golden("loss_grad")


def _restated(case, kind, name, k):
    x, y, lengths = lg.inputs(case)
    return lg.elementwise_grad(kind, x, y, lengths if name == "masked" else None, k)


@pytest.mark.parametrize("case,kind,name", lg.RUNS)
def test_restatement_matches_the_reference_float64(case, kind, name):
    for k in lg.UPSTREAM:
        key = lg.key(case, kind, name, k)
        ref = Z[key + "_64"]
        got = lg.stored(case, _restated(case, kind, name, k))
        assert got.shape == ref.shape and ref.dtype == np.float64
        if case == "d" and name == "masked":
            assert np.isnan(ref).all() and np.isnan(got).all() and np.isnan(Z[key + "_32"]).all()
            continue
        assert np.array_equal(got == 0, ref == 0) and not np.signbit(got[got == 0]).any()
        assert np.array_equal(Z[key + "_32"] == 0, ref == 0)
        rel = np.abs(got - ref)[ref != 0] / np.abs(ref[ref != 0])
        print(f"{key}: worst relative difference {rel.max():.3e} (bound {lg.F64_AGREE:.3e}) at {ref.size} elements")
        assert rel.max() <= lg.F64_AGREE


def test_bce_restatement_matches_the_reference_float64():
    x, y = eu.bce_inputs()
    for k in lg.UPSTREAM:
        ref = Z[f"e_bce_k{lg.UPSTREAM.index(k)}_64"]
        got = lg.bce_grad(x, y, k)
        err = np.abs(got - ref)
        print(f"bce k={k}: worst absolute difference {err.max():.3e}")
        assert (err <= lg.F64_AGREE * np.abs(ref) + lg.bce_abs(k, x.size)).all()


@pytest.mark.parametrize("case,kind,name", lg.RUNS)
def test_bounds_hold_for_the_reference_alone(case, kind, name):
    """got = float32(restated float64 gradient) passes both bounds of test_gpu_loss_grad.py."""
    for k in lg.UPSTREAM:
        key = lg.key(case, kind, name, k)
        g64 = lg.stored(case, _restated(case, kind, name, k))
        lg.check_gradient(g64.astype(np.float32), g64, Z[key + "_32"], Z[key + "_64"], what=key)


def test_bounds_hold_for_the_reference_alone_bce():
    x, y = eu.bce_inputs()
    for k in lg.UPSTREAM:
        key = f"e_bce_k{lg.UPSTREAM.index(k)}"
        g64 = lg.bce_grad(x, y, k)
        lg.check_gradient(g64.astype(np.float32), g64, Z[key + "_32"], Z[key + "_64"], lg.bce_abs(k, x.size), what=key)


def test_case_g_has_ties_and_h_is_no_multiple_of_four():
    x, y, lengths = lg.inputs("g")
    tie = lg.ties("g")
    assert 50 < tie.sum() < 400 and (x[tie] == y[tie]).all() and not tie[1].any() and not tie[2, 8:].any()
    assert x[0].size == 9225 > lg.CHUNK and x[0].size % 4 == 1
    assert (lg.elementwise_grad("l1", x, y, lengths, 1.0)[tie] == 0).all()
    assert np.prod(lg.CASES["h"][1][1:]) == 15
    idx = lg.sample_indices("g")
    assert {lg.CHUNK - 1, lg.CHUNK, 9224, 9225, 2 * 9225 + 8 * 1025 - 1, 2 * 9225 + 8 * 1025} <= set(idx.tolist())


def test_binding_declares_the_backward_entry_point():
    n = load_pkg("_native")
    assert "tts_loss_backward" in n.EXPORTS and n.TTS_LOSS_BCE == 2
    lib = n.load_library()
    assert lib.tts_loss_backward.restype is not None and len(lib.tts_loss_backward.argtypes) == 13


# ------------------------------------------------------------------ train_batch, sequencing on a CPU stand-in
class _LoggedAdam(torch.optim.Adam):
    def __init__(self, params, log, name, **kw):
        super().__init__(params, **kw)
        self._log, self._name = log, name

    def zero_grad(self, *a, **kw):
        self._log.append((self._name + ".zero_grad",))
        return super().zero_grad(*a, **kw)

    def step(self, *a, **kw):
        self._log.append((self._name + ".step",))
        return super().step(*a, **kw)


class _Scheduler:
    def __init__(self, log):
        self.log = log

    def step(self):
        self.log.append(("scheduler.step",))


def _run_train_batch(monkeypatch, c, scheduler=True):
    """train_batch on the CPU stand-in; the criteria, weight_decay and check_update are torch's and write to the
    log, together with whether the stopnet's weight has a gradient at that moment."""
    train = load_pkg("train")
    log = []
    model = tu.stand_in(c)
    stop_w = model.decoder.stopnet.weight
    forward = model.forward

    def logged_forward(*a, **kw):
        assert model.training and kw.keys() == {"speaker_ids"}
        log.append(("forward",))
        return forward(*a, **kw)

    def weight_decay(optimizer, wd):
        log.append(("weight_decay", optimizer._name, wd, stop_w.grad is not None))
        return tu.torch_weight_decay(optimizer, wd)

    def check_update(module, grad_clip):
        log.append(("check_update", "stopnet" if module is model.decoder.stopnet else "model", grad_clip,
                    stop_w.grad is not None))
        return tu.torch_check_update(module, grad_clip)

    model.forward = logged_forward
    monkeypatch.setattr(train, "_criteria", lambda cfg: tu.torch_criteria(cfg, log))
    monkeypatch.setattr(train, "weight_decay", weight_decay)
    monkeypatch.setattr(train, "check_update", check_update)
    opt = _LoggedAdam(model.parameters(), log, "optimizer", lr=c.lr)
    opt_st = None
    if c.separate_stopnet and c.stopnet:
        opt_st = _LoggedAdam(model.decoder.stopnet.parameters(), log, "optimizer_st", lr=c.lr)
    before = [p.detach().clone() for p in model.parameters()]
    out = train.train_batch(model, c, tu.batch(), opt, opt_st, _Scheduler(log) if scheduler else None)
    return out, log, model, before


def test_train_module_needs_no_gpu_to_import():
    train = load_pkg("train")
    assert callable(train.train_batch) and "train" in load_pkg().__all__


@pytest.mark.parametrize("model", ["Tacotron2", "Tacotron"])
def test_train_batch_sequence_with_a_separate_stopnet(monkeypatch, model):
    c = tu.config(model, lr_decay=True)
    out, log, net, before = _run_train_batch(monkeypatch, c)
    kind = "l1" if model == "Tacotron" else "mse"
    post = tu.D_LINEAR if model == "Tacotron" else tu.D
    assert log == [("scheduler.step",), ("optimizer.zero_grad",), ("optimizer_st.zero_grad",), ("forward",),
                   ("criterion_st", (tu.B, tu.T // tu.R)), ("criterion", kind, (tu.B, tu.T, tu.D), True),
                   ("criterion", kind, (tu.B, tu.T, post), True),
                   ("weight_decay", "optimizer", c.wd, False), ("check_update", "model", c.grad_clip, False),
                   ("optimizer.step",),
                   ("weight_decay", "optimizer_st", c.wd, True), ("check_update", "stopnet", 1.0, True),
                   ("optimizer_st.step",)]
    assert out["loss"] == out["decoder_loss"] + out["postnet_loss"] and out["stop_loss"] > 0
    assert out["current_lr"] == c.lr and float(out["grad_norm"]) > 0 and float(out["grad_norm_st"]) > 0
    assert all(not torch.equal(p, q) for p, q in zip(net.parameters(), before))
    assert out["stop_targets"].shape == (tu.B, tu.T // tu.R) and len(out["outputs"]) == 4


def test_train_batch_sequence_with_a_joint_stopnet(monkeypatch):
    c = tu.config(separate_stopnet=False, loss_masking=False)
    out, log, net, before = _run_train_batch(monkeypatch, c)
    assert log == [("optimizer.zero_grad",), ("forward",),  # lr_decay is off: the scheduler is not stepped
                   ("criterion_st", (tu.B, tu.T // tu.R)), ("criterion", "mse", (tu.B, tu.T, tu.D), False),
                   ("criterion", "mse", (tu.B, tu.T, tu.D), False),
                   ("weight_decay", "optimizer", c.wd, True), ("check_update", "model", c.grad_clip, True),
                   ("optimizer.step",)]
    assert out["loss"] == out["decoder_loss"] + out["postnet_loss"] + out["stop_loss"] and out["stop_loss"] > 0
    assert out["grad_norm_st"].dim() == 0 and float(out["grad_norm_st"]) == 0
    assert all(not torch.equal(p, q) for p, q in zip(net.parameters(), before))


@pytest.mark.parametrize("separate", [False, True])
def test_train_batch_sequence_without_a_stopnet(monkeypatch, separate):
    c = tu.config(stopnet=False, separate_stopnet=separate)
    out, log, net, before = _run_train_batch(monkeypatch, c, scheduler=False)
    assert log == [("optimizer.zero_grad",), ("forward",), ("criterion", "mse", (tu.B, tu.T, tu.D), True),
                   ("criterion", "mse", (tu.B, tu.T, tu.D), True),
                   ("weight_decay", "optimizer", c.wd, False), ("check_update", "model", c.grad_clip, False),
                   ("optimizer.step",)]
    assert out["stop_loss"] == 0.0 and out["loss"] == out["decoder_loss"] + out["postnet_loss"]
    assert float(out["grad_norm_st"]) == 0
    stop = [id(p) for p in net.decoder.stopnet.parameters()]
    for p, q in zip(net.parameters(), before):  # the stopnet had no gradient: the decay alone touched it
        assert p.grad is None if id(p) in stop else not torch.equal(p, q)


@pytest.mark.parametrize("kw", [dict(), dict(model="Tacotron"), dict(loss_masking=False),
                                dict(separate_stopnet=False), dict(stopnet=False)])
def test_torch_only_iterations_lower_the_loss(kw):
    losses = tu.torch_only_losses(tu.config(**kw), 10)
    print(kw, losses)
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
