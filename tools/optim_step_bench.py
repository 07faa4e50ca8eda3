"""The measurement behind profiles/optim_step.json (DESIGN "Training update"): one training update
(train.py:158-160) on a parameter set with the element counts of the Tacotron2 that bench.py builds (read
from the model's state dict; BatchNorm buffers are no parameters), as

  (i)   optim.Adam.step_fused(wd, grad_clip)                                   one norm reduction, one pass
  (ii)  generic_utils.weight_decay, check_update, optim.Adam.step              the three stand-alone calls
  (iii) the reference's weight_decay loop, clip_grad_norm_ with the reference's inf test, and
        torch.optim.Adam.step with its defaults, PyTorch-ROCm ops on the same device

    python tools/optim_step_bench.py OUT.json

Each is timed per call with device events over REPS calls after WARMUP (launches, the table upload and every
host wait the variant has included), median / min / max.  (i) is also enqueued through the C-ABI REPS times
back to back with a prebuilt table between two events: the device's own time per update, host preparation
off the path; its bytes over that time is the achieved bandwidth.  wd = 1e-6 and grad_clip = 1.0 are the
reference config's; the gradients' norm is below 1, as in a fine-tuning run past its first steps, so the clip
does not scale (an active clip adds one 4-byte write of g per element to (i)).  Parameters, gradients and
state are 16 bytes per element, 450 MB: more than the 256 MiB Infinity Cache.  The three variants' results
are compared after the first call.
"""
import ctypes
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "your-voice-tts_amd"
WARMUP, REPS = 5, 50
WD, GRAD_CLIP, LR = 1e-6, 1.0, 1e-4


def element_counts():
    gu = importlib.import_module(PKG + ".generic_utils")
    model = gu.setup_model(130, gu.default_config())
    return [(k, v.numel()) for k, v in model.state_dict().items()
            if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))]


def timed(fn):
    import torch
    ts = []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ts.append(a.elapsed_time(b) * 1e3)
    ts = sorted(ts)
    return dict(event_us_median=ts[len(ts) // 2], event_us_min=ts[0], event_us_max=ts[-1], calls=WARMUP + REPS)


def run(out):
    import numpy as np
    import torch
    optim = importlib.import_module(PKG + ".optim")
    gu = importlib.import_module(PKG + ".generic_utils")
    native = importlib.import_module(PKG + "._native")
    counts = element_counts()
    n_elem = sum(n for _, n in counts)
    g = torch.Generator().manual_seed(0)
    p0 = [0.1 * torch.randn(n, generator=g) for _, n in counts]
    scale = 0.5 / np.sqrt(n_elem)  # norm ~ 0.5: below grad_clip
    g0 = [scale * torch.randn(n, generator=g) for _, n in counts]

    def param_set():
        ps = [torch.nn.Parameter(t.cuda()) for t in p0]
        for P, t in zip(ps, g0):
            P.grad = t.cuda()
        return ps

    res = dict(device=torch.cuda.get_device_name(0), tensors=len(counts), elements=n_elem,
               largest_tensor=max(n for _, n in counts), smallest_tensor=min(n for _, n in counts),
               chunk=optim.CHUNK, chunks=sum(-(-n // optim.CHUNK) for _, n in counts), warmup=WARMUP, reps=REPS,
               wd=WD, grad_clip=GRAD_CLIP, lr=LR)

    # (i) fused
    ps_f = param_set()
    opt_f = optim.Adam(ps_f, lr=LR)
    norm_f, _ = opt_f.step_fused(WD, GRAD_CLIP)
    first_f = [P.detach().clone() for P in ps_f]
    res["grad_norm"] = float(norm_f)
    assert float(norm_f) < GRAD_CLIP
    res["step_fused"] = timed(lambda: opt_f.step_fused(WD, GRAD_CLIP))
    res["step_fused"]["bytes"] = 32 * n_elem  # norm: g; update: p, g, m, v read, p, m, v written

    # (i) again, device time: the C-ABI call back to back, table prebuilt (the engine's own, just used)
    lib, h = opt_f._engine._h
    table, n = opt_f._engine._table, len(ps_f)
    for i, P in enumerate(ps_f):
        table[i].step = int(opt_f.state[P]["step"]) + 1
    n64 = torch.empty(2, dtype=torch.float64, device="cuda")
    n32 = torch.empty(2, dtype=torch.float32, device="cuda")
    s = native.stream_handle()
    args = (h, table, n, LR, 0.9, 0.999, 1e-8, WD, GRAD_CLIP, ctypes.c_void_p(n64.data_ptr()),
            ctypes.c_void_p(n32.data_ptr()), s)
    for _ in range(WARMUP):
        native.check(lib.tts_optim_step(*args), "tts_optim_step")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        native.check(lib.tts_optim_step(*args), "tts_optim_step")
    b.record()
    b.synchronize()
    us = a.elapsed_time(b) * 1e3 / REPS
    res["step_fused_device"] = dict(us_per_call=us, calls_back_to_back=REPS, bytes=32 * n_elem,
                                    TB_per_s=32 * n_elem / (us * 1e-6) / 1e12)

    # (ii) the three stand-alone calls
    ps_u = param_set()
    opt_u = optim.Adam(ps_u, lr=LR)

    def three_calls():
        gu.weight_decay(opt_u, WD)
        gu.check_update(ps_u, GRAD_CLIP)
        opt_u.step()

    three_calls()
    assert all(torch.equal(x, y.detach()) for x, y in zip(first_f, ps_u)), "fused and unfused differ"
    res["three_calls"] = timed(three_calls)
    res["three_calls"]["bytes"] = 40 * n_elem  # decay: p read and written; norm: g; Adam: 16 read, 12 written

    # (iii) torch on the same device, the reference's own way
    ps_t = param_set()
    opt_t = torch.optim.Adam(ps_t, lr=LR, weight_decay=0)

    def reference_way():
        for group in opt_t.param_groups:  # generic_utils.py:178-181
            for param in group["params"]:
                param.data = param.data.add(param.data, alpha=-WD * group["lr"])
        grad_norm = torch.nn.utils.clip_grad_norm_(ps_t, GRAD_CLIP)  # generic_utils.py:158-159
        if np.isinf(grad_norm.item()):
            raise RuntimeError("inf")
        opt_t.step()

    reference_way()
    diff = max(float((x - y.detach()).abs().max()) for x, y in zip(first_f, ps_t))
    res["max_abs_difference_to_torch_after_one_update"] = diff
    assert diff < 1e-6, diff  # (|dp| = lr = 1e-4; the float32 results agree to rounding)
    res["torch_reference_way"] = timed(reference_way)

    for k in ("step_fused", "three_calls"):
        res[k]["TB_per_s_of_the_call"] = res[k]["bytes"] / (res[k]["event_us_median"] * 1e-6) / 1e12
    res["ratio_torch_over_step_fused"] = res["torch_reference_way"]["event_us_median"] / res["step_fused"]["event_us_median"]
    res["ratio_torch_over_three_calls"] = res["torch_reference_way"]["event_us_median"] / res["three_calls"]["event_us_median"]
    res["ratio_torch_over_step_fused_device"] = res["torch_reference_way"]["event_us_median"] / us
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    run(sys.argv[1])
