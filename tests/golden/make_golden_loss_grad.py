"""Generate tests/golden/loss_grad.npz by running the REFERENCE loss modules with autograd.

Run in the build container only (needs /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_golden_loss_grad.py

Built as make_golden_eval.py is: make_golden's stubs, then ``layers.losses`` from the reference.
``L1LossMasked``, ``MSELossMasked`` (layers/losses.py), ``nn.L1Loss``, ``nn.MSELoss`` and ``nn.BCEWithLogitsLoss``
on the seeded inputs of tests/loss_grad_util.py with ``requires_grad_(True)``, once in float32 and once with the
tensors cast to float64, with upstream gradients 1 and 0.375 (the second through ``(0.375 * loss).backward()``);
the input's ``.grad`` is what is stored.  Cases a, c, d, h and BCE in full; b and g at the index sample of
``loss_grad_util.sample_indices`` (every chunk edge and every n[b] +- 4 elements, 2000 seeded indices).  Only
seeds (in loss_grad_util.py, eval_util.py) and results are stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the stubs, REF)
import eval_util as eu  # noqa: E402
import loss_grad_util as lg  # noqa: E402  (the inputs, the index sample)


def _grad(fn, x, y, k, dtype):
    import torch
    x = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = torch.from_numpy(y).to(dtype)
    loss = fn(x, y)
    assert loss.dtype == dtype
    (loss if k == 1.0 else k * loss).backward()
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    return x.grad.numpy()


def main():
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    import torch
    from torch import nn
    from layers.losses import L1LossMasked, MSELossMasked
    masked = dict(l1=L1LossMasked(), mse=MSELossMasked())
    plain = dict(l1=nn.L1Loss(), mse=nn.MSELoss())
    out = {}
    for case, kind, name in lg.RUNS:
        x, y, lengths = lg.inputs(case)
        if name == "masked":
            fn = lambda a, b: masked[kind](a, b, torch.LongTensor(lengths))
        else:
            fn = lambda a, b: plain[kind](a, b)
        for k in lg.UPSTREAM:
            key = lg.key(case, kind, name, k)
            g32, g64 = _grad(fn, x, y, k, torch.float32), _grad(fn, x, y, k, torch.float64)
            out[key + "_32"], out[key + "_64"] = lg.stored(case, g32), lg.stored(case, g64)
            print(f"{key}: {out[key + '_64'].size} of {g64.size} elements stored, "
                  f"{int(np.isnan(g64).sum())} NaN, {int((g64 == 0).sum())} zero, max |g64| {np.nanmax(np.abs(g64)) if not np.isnan(g64).all() else float('nan'):.6g}")
    x, y = eu.bce_inputs()
    for k in lg.UPSTREAM:
        key = f"e_bce_k{lg.UPSTREAM.index(k)}"
        out[key + "_32"] = _grad(nn.BCEWithLogitsLoss(), x, y, k, torch.float32)
        out[key + "_64"] = _grad(nn.BCEWithLogitsLoss(), x, y, k, torch.float64)
        print(f"{key}: {x.size} elements stored, first ten f64 {out[key + '_64'][:10]}")
    path = os.path.join(HERE, "loss_grad.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
