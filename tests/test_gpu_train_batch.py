"""``train.train_batch`` on the device against the same iteration written out by hand with the package's criteria,
``.backward()`` and ``optim.Adam.step_fused`` (train.py:92-169), on the stand-in model and the fixed batch of
train_util.py: bitwise the parameters, the Adam state, the losses and the gradient norms, for Tacotron2 (MSE) and
Tacotron (L1 against ``linear``), masked and not, with a separate, a joint and no stopnet.  The by-hand sequence is
first run twice and compared with itself, so an op of the stand-in whose backward is not run-to-run
deterministic shows up as that and not as a difference of ``train_batch``.
"""
import numpy as np
import pytest
import torch

import eval_util as eu
import train_util as tu
from conftest import load_pkg

pytestmark = pytest.mark.gpu
CONFIGS = {"tacotron2": dict(), "tacotron": dict(model="Tacotron"), "unmasked": dict(loss_masking=False),
           "joint_stopnet": dict(separate_stopnet=False), "no_stopnet": dict(stopnet=False),
           "tacotron_joint_unmasked": dict(model="Tacotron", separate_stopnet=False, loss_masking=False)}


def _setup(c, adam=None):
    """(model, optimizer, optimizer_st) as train.py:450-459 makes them, on the device."""
    adam = adam or load_pkg("optim").Adam
    model = tu.stand_in(c, "cuda")
    optimizer = adam(model.parameters(), lr=c.lr, weight_decay=0)
    optimizer_st = None
    if c.stopnet and c.separate_stopnet:
        optimizer_st = adam(model.decoder.stopnet.parameters(), lr=c.lr, weight_decay=0)
    return model, optimizer, optimizer_st


def _by_hand(model, c, batch, optimizer, optimizer_st):
    lo, gu = load_pkg("losses"), load_pkg("generic_utils")
    text, text_lengths, _, linear, mel, mel_lengths, stop_targets, _ = batch
    tacotron = c.model in ("Tacotron", "TacotronGST")
    stop_targets = (stop_targets.view(text.shape[0], stop_targets.size(1) // c.r, -1).sum(2) > 0.0).float()
    optimizer.zero_grad()
    if optimizer_st:
        optimizer_st.zero_grad()
    dec, post, _, stop = model(text.cuda(), text_lengths.cuda(), mel, speaker_ids=None)
    if c.loss_masking:
        criterion, length = (lo.L1LossMasked() if tacotron else lo.MSELossMasked()), (mel_lengths,)
    else:
        criterion, length = (lo.L1Loss() if tacotron else lo.MSELoss()), ()
    values = dict(stop_loss=0.0)
    if c.stopnet:
        criterion_st = lo.BCEWithLogitsLoss()
        stop_loss = criterion_st(stop, stop_targets)
        values["stop_loss"] = criterion_st.last_value
    decoder_loss = criterion(dec, mel, *length)
    values["decoder_loss"] = criterion.last_value
    postnet_loss = criterion(post, linear if tacotron else mel, *length)
    values["postnet_loss"] = criterion.last_value
    loss = decoder_loss + postnet_loss
    values["loss"] = values["decoder_loss"] + values["postnet_loss"]
    if c.stopnet and not c.separate_stopnet:
        loss = loss + stop_loss
        values["loss"] += values["stop_loss"]
    loss.backward()
    values["grad_norm"], values["current_lr"] = optimizer.step_fused(c.wd, c.grad_clip)
    values["grad_norm_st"] = torch.zeros((), device="cuda")
    if c.stopnet and c.separate_stopnet:
        stop_loss.backward()
        gu.weight_decay(optimizer_st, c.wd)
        values["grad_norm_st"], _ = gu.check_update(model.decoder.stopnet, 1.0)
        optimizer_st.step()
    return values


def _state(model, *optimizers):
    out = {"p." + k: v.detach().clone() for k, v in model.named_parameters()}
    for i, opt in enumerate(o for o in optimizers if o is not None):
        for j, p in enumerate(opt.param_groups[0]["params"]):
            for k, v in opt.state[p].items():
                out[f"opt{i}.{j}.{k}"] = torch.as_tensor(v).detach().clone()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k


SCALARS = ("decoder_loss", "postnet_loss", "stop_loss", "loss", "current_lr")


@pytest.mark.parametrize("name", CONFIGS)
def test_gpu_train_batch_is_the_iteration_by_hand(name):
    c = tu.config(**CONFIGS[name])
    batch = tu.batch("cuda")
    runs = []
    for _ in range(2):
        model, opt, opt_st = _setup(c)
        values = _by_hand(model, c, batch, opt, opt_st)
        runs.append((values, _state(model, opt, opt_st)))
    _same(runs[0][1], runs[1][1])  # the stand-in is run-to-run deterministic
    assert [runs[0][0][k] for k in SCALARS] == [runs[1][0][k] for k in SCALARS]

    model, opt, opt_st = _setup(c)
    before = _state(model)
    out = load_pkg("train").train_batch(model, c, batch, opt, opt_st)
    want, want_state = runs[0]
    _same(_state(model, opt, opt_st), want_state)
    assert [out[k] for k in SCALARS] == [want[k] for k in SCALARS]
    for k in ("grad_norm", "grad_norm_st"):
        assert out[k].dim() == 0 and torch.equal(out[k].cpu(), want[k].cpu()), k
    assert float(out["grad_norm"]) > 0 and (float(out["grad_norm_st"]) > 0) == (c.stopnet and c.separate_stopnet)
    after = _state(model)
    moved = [k for k in after if not torch.equal(after[k], before[k])]
    assert len(moved) >= len(after) - 2  # (all but a stopnet that got no gradient: its bias is 0, which the decay keeps)

    # the returned losses are the criteria's fp64 values of the returned outputs
    dec, post, _, stop = (t.detach().cpu().numpy() for t in out["outputs"])
    tacotron = c.model == "Tacotron"
    kind = "l1" if tacotron else "mse"
    lengths = tu.MEL_LENGTHS if c.loss_masking else None
    mel, linear = batch[4].cpu().numpy(), batch[3].cpu().numpy()
    ref, count, _ = eu.elementwise_loss(kind, dec, mel, lengths)
    assert eu.within(out["decoder_loss"], ref, count)
    ref, count, _ = eu.elementwise_loss(kind, post, linear if tacotron else mel, lengths)
    assert eu.within(out["postnet_loss"], ref, count)
    assert out["stop_targets"].shape == (tu.B, tu.T // tu.R) and out["stop_targets"].is_cuda
    if c.stopnet:
        ref, n = eu.bce_with_logits(stop, out["stop_targets"].cpu().numpy())
        assert eu.within(out["stop_loss"], ref, n)
    else:
        assert out["stop_loss"] == 0.0


@pytest.mark.parametrize("name", ["tacotron2", "tacotron_joint_unmasked"])
def test_gpu_ten_iterations_lower_the_loss(name):
    """test_loss_grad_cpu.py asserts the same of the torch-only sequence on the CPU."""
    c = tu.config(**CONFIGS[name])
    batch = tu.batch("cuda")
    model, opt, opt_st = _setup(c)
    train = load_pkg("train")
    losses = [train.train_batch(model, c, batch, opt, opt_st)["loss"] for _ in range(10)]
    print(name, losses, tu.torch_only_losses(c, 10))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))


@pytest.mark.parametrize("separate", [False, True])
def test_gpu_train_batch_with_a_torch_optimizer(separate):
    """A plain torch.optim.Adam takes the branch of weight_decay(); check_update(); optimizer.step()."""
    c = tu.config(separate_stopnet=separate)
    model, opt, opt_st = _setup(c, torch.optim.Adam)
    before = _state(model)
    out = load_pkg("train").train_batch(model, c, tu.batch("cuda"), opt, opt_st)
    after = _state(model)
    for k in after:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(after[k], before[k]), k
    assert out["current_lr"] == c.lr and np.isfinite(out["loss"]) and float(out["grad_norm"]) > 0
    # the same iteration with the package's Adam: the same losses, and the update of one Adam step apart at most
    model2, opt2, opt_st2 = _setup(c)
    out2 = load_pkg("train").train_batch(model2, c, tu.batch("cuda"), opt2, opt_st2)
    assert [out2[k] for k in SCALARS] == [out[k] for k in SCALARS]
    for k, v in _state(model2).items():
        assert float((v - after[k]).abs().max()) <= 1e-3 * c.lr, k
