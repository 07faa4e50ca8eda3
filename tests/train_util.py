"""Shared by test_loss_grad_cpu.py and test_gpu_train_batch.py: a stand-in for the reference's models with their
forward signature and four outputs, one fixed collated batch, a config, and the training iteration of
train.py:92-169 written with torch alone (torch criteria by the reference's formulas, ``torch.optim.Adam``).

The stand-in uses only ops whose backward is run-to-run deterministic on the device: elementwise ops, broadcasts
and plain reductions (no embedding, no scatter, no GEMM).  Its "decoder" scales the teacher-forcing mel, so the
loss falls as the scale approaches 1.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional

B, T, D, D_LINEAR, R, TEXT = 3, 10, 8, 12, 2, 6
MEL_LENGTHS = [10, 7, 4]
TEXT_LENGTHS = [6, 5, 3]
LR = 0.01


class Config(dict):
    __getattr__ = dict.__getitem__


def config(model="Tacotron2", **kw):
    c = Config(model=model, r=R, wd=1e-6, grad_clip=1.0, lr=LR, lr_decay=False, loss_masking=True, stopnet=True,
               separate_stopnet=True, use_speaker_embedding=False)
    c.update(kw)
    return c


def batch(device="cpu"):
    """A batch as datasets.collate_fn returns it: the features and stop targets on ``device``, the rest on the host."""
    g = np.random.Generator(np.random.PCG64(301))
    mel = g.uniform(0.0, 1.0, (B, T, D)).astype(np.float32)
    linear = g.uniform(0.0, 1.0, (B, T, D_LINEAR)).astype(np.float32)
    stop = np.zeros((B, T), np.float32)
    for b, n in enumerate(MEL_LENGTHS):
        mel[b, n:], linear[b, n:] = 0.0, 0.0
        stop[b, n - 1:] = 1.0
    text = g.integers(1, 100, (B, TEXT))
    for b, n in enumerate(TEXT_LENGTHS):
        text[b, n:] = 0
    return (torch.from_numpy(text), torch.LongTensor(TEXT_LENGTHS), [f"spk{b}" for b in range(B)],
            torch.from_numpy(linear).to(device), torch.from_numpy(mel).to(device), torch.LongTensor(MEL_LENGTHS),
            torch.from_numpy(stop).to(device), [f"item{b}.wav" for b in range(B)])


class Dot(nn.Module):
    """``(h * weight).sum(-1) + bias``: a Linear to one unit, from an elementwise product and a plain reduction."""

    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.linspace(-0.3, 0.3, n))
        self.bias = nn.Parameter(torch.zeros(1))

    def forward(self, h):
        return (h * self.weight).sum(-1) + self.bias


class StandIn(nn.Module):
    """forward(text, text_lengths, mel, speaker_ids=None) -> (decoder_output [B, T, D], postnet_output
    [B, T, postnet_dim], alignments [B, T / r, L], stop_tokens [B, T / r]); ``decoder.stopnet`` reads the decoder
    output detached when ``separate_stopnet``, as the reference's decoders do."""

    def __init__(self, postnet_dim=D, separate_stopnet=True, r=R):
        super().__init__()
        self.r, self.separate_stopnet, self.postnet_dim = r, separate_stopnet, postnet_dim
        self.text_scale = nn.Parameter(torch.tensor([0.01]))
        self.dec_w = nn.Parameter(torch.linspace(0.4, 0.6, D))
        self.dec_b = nn.Parameter(torch.zeros(D))
        self.post_w = nn.Parameter(torch.linspace(0.1, 0.3, postnet_dim))
        self.post_b = nn.Parameter(torch.zeros(postnet_dim))
        self.decoder = nn.Module()
        self.decoder.stopnet = Dot(D * r)

    def forward(self, text, text_lengths, mel, speaker_ids=None):
        nb, nt, nd = mel.shape
        t = (text.float().sum(1) / text_lengths.float() / 100.0)[:, None, None] * self.text_scale
        dec = mel * self.dec_w + self.dec_b + t
        if self.postnet_dim == nd:
            post = dec + dec * self.post_w + self.post_b
        else:
            post = dec.mean(2, keepdim=True) * self.post_w + self.post_b
        h = dec.reshape(nb, nt // self.r, nd * self.r)
        stop = self.decoder.stopnet(h.detach() if self.separate_stopnet else h)
        return dec, post, torch.zeros(nb, nt // self.r, text.shape[1], device=mel.device), stop


def stand_in(c, device="cpu"):
    tacotron = c.model in ("Tacotron", "TacotronGST")
    return StandIn(D_LINEAR if tacotron else D, c.separate_stopnet and c.stopnet).to(device).train()


# ------------------------------------------------------------------ torch criteria by the reference's formulas
class TorchCriterion:
    """layers/losses.py:27-32, 56-61 (lengths given) or nn.L1Loss / nn.MSELoss; ``last_value`` as the package's
    criteria have it; every call is appended to ``log``."""

    def __init__(self, kind, log=None):
        self.kind, self.log, self.last_value = kind, log if log is not None else [], None

    def __call__(self, input, target, length=None):
        f = functional.l1_loss if self.kind == "l1" else functional.mse_loss
        if length is None:
            loss = f(input, target)
        else:
            mask = (torch.arange(target.size(1))[None, :] < torch.as_tensor(length)[:, None])
            mask = mask.to(input.device).unsqueeze(2).float().expand_as(input)
            loss = f(input * mask, target * mask, reduction="sum") / mask.sum()
        self.last_value = float(loss.detach())
        self.log.append(("criterion", self.kind, tuple(input.shape), length is not None))
        return loss


class TorchBCE:
    def __init__(self, log=None):
        self.log, self.last_value = log if log is not None else [], None

    def __call__(self, input, target):
        loss = functional.binary_cross_entropy_with_logits(input, target)
        self.last_value = float(loss.detach())
        self.log.append(("criterion_st", tuple(input.shape)))
        return loss


def torch_criteria(c, log=None):
    """What evaluate._criteria(c) returns, in torch."""
    kind = "l1" if c.model in ("Tacotron", "TacotronGST") else "mse"
    return TorchCriterion(kind, log), (TorchBCE(log) if c.stopnet else None)


def torch_weight_decay(optimizer, wd):  # utils/generic_utils.py:174-182
    for group in optimizer.param_groups:
        current_lr = group["lr"]
        for p in group["params"]:
            p.data = p.data.add(p.data, alpha=-wd * current_lr)
    return optimizer, current_lr


def torch_check_update(model, grad_clip):  # utils/generic_utils.py:155-162
    params = model.parameters() if hasattr(model, "parameters") else model
    return torch.nn.utils.clip_grad_norm_(params, grad_clip), False


def torch_only_losses(c, iterations):
    """``iterations`` of train.py:92-169 on the CPU with torch alone, on the fixed batch: the ``loss`` of each."""
    model = stand_in(c)
    optimizer = torch.optim.Adam(model.parameters(), lr=c.lr, weight_decay=0)
    separate = c.separate_stopnet and c.stopnet
    optimizer_st = torch.optim.Adam(model.decoder.stopnet.parameters(), lr=c.lr, weight_decay=0) if separate else None
    text, text_lengths, _, linear, mel, mel_lengths, stop_targets, _ = batch()
    stop_targets = (stop_targets.view(B, T // c.r, -1).sum(2) > 0.0).float()
    criterion, criterion_st = torch_criteria(c)
    length = (mel_lengths,) if c.loss_masking else ()
    out = []
    for _ in range(iterations):
        optimizer.zero_grad()
        if optimizer_st:
            optimizer_st.zero_grad()
        dec, post, _, stop = model(text, text_lengths, mel)
        stop_loss = criterion_st(stop, stop_targets) if criterion_st else None
        loss = criterion(dec, mel, *length) + criterion(post, linear if criterion.kind == "l1" else mel, *length)
        if c.stopnet and not separate:
            loss = loss + stop_loss
        loss.backward()
        torch_weight_decay(optimizer, c.wd)
        torch_check_update(model, c.grad_clip)
        optimizer.step()
        if separate:
            stop_loss.backward()
            torch_weight_decay(optimizer_st, c.wd)
            torch_check_update(model.decoder.stopnet, 1.0)
            optimizer_st.step()
        out.append(float(loss.detach()))
    return out
