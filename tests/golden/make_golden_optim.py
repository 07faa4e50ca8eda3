"""Generate tests/golden/optim.npz by running the REFERENCE training-update helpers with the installed torch.

Run in the build container only (needs /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_golden_optim.py

The reference's ``utils/generic_utils.py`` is imported as it stands (text dependencies stubbed as the other
generators stub them) and its ``weight_decay``, ``check_update``, ``NoamLR`` and ``lr_decay`` run on CPU
together with ``torch.optim.Adam(lr, weight_decay=0, foreach=False)``, train.py:158-160 as written there,
three consecutive iterations per case of tests/optim_util.py (tensor set, seeds, cases (a)-(e)).  In case
(d) the state is restored at step 1000 and ``NoamLR(last_epoch=999)`` steps before every iteration
(train.py:119-120, 501-505).

Stored, per case and iteration: the norm ``check_update`` returned (float32), ``current_lr``, the steps, and
torch's p, g, m, v AT THE SAMPLED ELEMENTS of each tensor (``optim_util.sample_indices``: all of a small
tensor; both ends, both sides of every chunk boundary and 96 seeded positions of a large one).  The update
is elementwise, so the sample of a full run is exactly what a test needs there; the full arrays of twelve
iterations would be 24 MB of random bits, and the inputs are regenerated from the seeds.  Also the schedule
values of ``lr_decay`` and ``NoamLR`` at the steps of ``optim_util.SCHEDULE_STEPS``.
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the stubs, REF)
import optim_util as ou  # noqa: E402  (the inputs)


def tensors(arrays):
    """Parameters over the arrays; the VIEW one at element offset 1 of a larger buffer."""
    import torch
    out = []
    for i, a in enumerate(arrays):
        if i == ou.VIEW:
            buf = torch.zeros(a.size + 8)
            buf[1:1 + a.size] = torch.from_numpy(a)
            out.append(buf[1:1 + a.size])
        else:
            out.append(torch.from_numpy(a.copy()))
    return out


def run_case(case, out, gu):
    import torch
    cfg = ou.CASES[case]
    p0, m0, v0, steps0 = ou.initial_state(case)
    params = [torch.nn.Parameter(t) for t in tensors(p0)]
    optimizer = torch.optim.Adam(params, lr=cfg["lr"], weight_decay=0, foreach=False)
    if cfg["step0"]:
        for P, m, v, s in zip(params, tensors(m0), tensors(v0), steps0):
            optimizer.state[P] = dict(step=torch.tensor(float(s)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    scheduler = None
    if cfg["noam"]:
        for group in optimizer.param_groups:
            group["initial_lr"] = cfg["lr"]
        scheduler = gu.NoamLR(optimizer, warmup_steps=ou.WARMUP, last_epoch=cfg["step0"] - 1)
    idx = [ou.sample_indices(n) for n in ou.SIZES]
    model = types.SimpleNamespace(parameters=lambda: params)  # what check_update asks of a model
    for it in range(ou.ITERATIONS):
        if scheduler is not None:
            scheduler.step()
        for P, g in zip(params, tensors_or_none(ou.gradients(case, it))):
            P.grad = g
        optimizer, current_lr = gu.weight_decay(optimizer, cfg["wd"])
        grad_norm, skip_flag = gu.check_update(model, cfg["grad_clip"])
        optimizer.step()
        assert not skip_flag and grad_norm.dtype == torch.float32
        key = f"{case}{it}"
        out[key + "_norm"] = np.float32(grad_norm.item())
        out[key + "_lr"] = np.float64(current_lr)
        out[key + "_steps"] = np.array([int(optimizer.state[P]["step"]) if P in optimizer.state and optimizer.state[P]
                                        else 0 for P in params])
        for i, P in enumerate(params):
            st = optimizer.state[P] if P in optimizer.state else {}
            out[f"{key}_p{i}"] = P.detach().numpy()[idx[i]].copy()
            if P.grad is not None:
                out[f"{key}_g{i}"] = P.grad.numpy()[idx[i]].copy()
            if st:
                out[f"{key}_m{i}"] = st["exp_avg"].numpy()[idx[i]].copy()
                out[f"{key}_v{i}"] = st["exp_avg_sq"].numpy()[idx[i]].copy()
        print(f"{key}: norm {grad_norm.item():.9g} lr {current_lr!r} steps {out[key + '_steps'].tolist()}")


def tensors_or_none(arrays):
    import torch
    return [None if a is None else torch.from_numpy(a.copy()) for a in arrays]


def schedules(out, gu):
    import torch
    out["lr_decay"] = np.array([gu.lr_decay(1e-3, s, ou.WARMUP) for s in ou.SCHEDULE_STEPS], np.float64)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sch = gu.NoamLR(opt, warmup_steps=ou.WARMUP, last_epoch=-1)  # (its constructor takes step 0)
    vals = {0: opt.param_groups[0]["lr"]}
    for s in range(1, max(ou.SCHEDULE_STEPS) + 1):
        sch.step()
        if s in ou.SCHEDULE_STEPS:
            vals[s] = opt.param_groups[0]["lr"]
    out["noam_lr"] = np.array([vals[s] for s in ou.SCHEDULE_STEPS], np.float64)
    print("lr_decay", out["lr_decay"].tolist(), "\nNoamLR", out["noam_lr"].tolist())


def main():
    warnings.filterwarnings("ignore")  # the deprecated add(Number, Tensor) overload, scheduler.step() order
    mg._stub_text_deps()
    sys.path.insert(0, mg.REF)
    from utils import generic_utils as gu
    out = {}
    for case in ou.CASES:
        run_case(case, out, gu)
    schedules(out, gu)
    path = os.path.join(HERE, "optim.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 400 << 10


if __name__ == "__main__":
    main()
