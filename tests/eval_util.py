"""Shared by tests/golden/make_golden_eval.py, test_eval_cpu.py and the GPU tests of the evaluation path:
the inputs of the eval.npz fixture (regenerated from seeds, never stored), a plain float64 torch
restatement of the five losses and of the per-r stop-target grouping, and the error bounds.

The fp64 bound: a float64 sum of N terms, each formed with at most one rounding, in ANY order lies within
(N - 1) u of the exact sum relative to the sum of |terms| (all terms here are >= 0, so relative to the sum
itself), u = 2^-53; two such sums (the reference's and the one under test), the term's own rounding and the
final division stay within (N + 4) * 2^-52 of each other.
"""
import numpy as np
import torch

ITEMS = [(8000, 4 * 275 + 37, 5), (20000, 7 * 275 + 100, 9), (12000, 6 * 275 - 1, 7), (3000, 2 * 275, 4)]
RS = (1, 2, 5)

# name -> (seed, (B, T, D), lengths or None)
LOSS_CASES = {
    "a": (101, (5, 13, 80), [13, 1, 7, 20, 4]),     # one length above T
    "b": (102, (3, 37, 1025), [37, 5, 36]),         # odd D, misaligned bases, several chunks per sentence
    "c": (103, (2, 3, 1), None),
    "d": (104, (3, 4, 5), [0, 0, 0]),               # no valid row: NaN
}
BCE_SEED, BCE_N = 105, 257


def collate_items(pcm):
    """The four items of the collate fixture from example_1.wav's int16 samples: float32 excerpts, distinct
    text lengths that are not in wav-length order."""
    x = (np.asarray(pcm).astype(np.float64) / 32768.0).astype(np.float32)
    return [dict(text=((np.arange(L) * 7 + 11 * (i + 1)) % 120 + 2).astype(np.int32), wav=x[off:off + n].copy(),
                 item_idx=f"item{i}.wav", speaker_name=f"spk{i}") for i, (off, n, L) in enumerate(ITEMS)]


def loss_inputs(case):
    seed, shape, lengths = LOSS_CASES[case]
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal(shape).astype(np.float32)
    y = g.uniform(-1.0, 1.0, shape).astype(np.float32)
    return x, y, lengths


def bce_inputs():
    g = np.random.Generator(np.random.PCG64(BCE_SEED))
    x = (3.0 * g.standard_normal(BCE_N)).astype(np.float32)
    y = g.integers(0, 2, BCE_N).astype(np.float32)
    x[:10] = [100, -100, 50, -50, 0, 100, -100, 50, -50, 0]
    y[:5], y[5:10] = 1.0, 0.0
    return x, y


def fp64_bound(n_terms):
    return (n_terms + 4) * 2.0 ** -52


def sentence_terms(shape, lengths, b):
    """Number of terms sentence b of a [B, T, D] batch contributes."""
    return (shape[1] if lengths is None else min(lengths[b], shape[1])) * shape[2]


def within(value, ref, n_terms):
    """value is within the fp64 bound of ref, relative (NaN matches NaN)."""
    if np.isnan(ref):
        return bool(np.isnan(value))
    return abs(value - ref) <= fp64_bound(n_terms) * abs(ref)


# ------------------------------------------------------------------ the losses, restated in float64
def elementwise_loss(kind, x, y, lengths=None):
    """L1LossMasked / MSELossMasked (lengths given) or nn.L1Loss / nn.MSELoss (None) on [B, T, D] in
    float64.  Returns (loss, number of terms, per-sentence sums)."""
    x = torch.as_tensor(x).double()
    y = torch.as_tensor(y).double()
    B, T, D = x.shape
    rows = torch.full((B,), T) if lengths is None else torch.as_tensor(lengths).clamp(max=T)
    mask = (torch.arange(T)[None, :] < rows[:, None])[:, :, None].expand_as(x)
    d = (x - y)[mask]
    terms = torch.zeros_like(x)
    terms[mask] = d.abs() if kind == "l1" else d * d
    count = int(rows.sum()) * D
    total = terms.sum()
    loss = float(total) / count if count else float("nan")
    return loss, count, terms.sum((1, 2)).numpy()


def bce_with_logits(x, y):
    x = torch.as_tensor(x).double().reshape(-1)
    y = torch.as_tensor(y).double().reshape(-1)
    terms = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    return float(terms.sum()) / x.numel(), x.numel()


def group_stop_targets(stop_targets, r):
    """train.py:306-309: one target per decoder step, 1 when any of its r frames' targets is."""
    s = np.asarray(stop_targets)
    return (s.reshape(s.shape[0], s.shape[1] // r, r).sum(2) > 0).astype(np.float32)
