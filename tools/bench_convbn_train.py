"""The measurement behind profiles/convbn_train.json (DESIGN "Trainable conv-BN block"): forward + every gradient of
the reference's two conv-BN stacks at a training shape (tests/convbn_train_util.py: BENCH), the three encoder
blocks (512 -> 512, relu) at B = 32, T = 150 and the five Postnet blocks (80 -> 512 -> 512 -> 512 -> 512 -> 80) at
B = 32, T = 600, as (a) layers.ConvBNBlock (tts_convbn_forward / tts_convbn_backward; its dropout mask drawn with
torch.rand on the device, inside the timed region) and (b) the same blocks as torch ``nn.Sequential(Conv1d,
BatchNorm1d, [ReLU | Tanh], Dropout)`` on the same device, the same weights and the same data.  Both produce out,
grad_x and the four parameter gradients of every block.

    python tools/bench_convbn_train.py run OUT.json
    rocprofv3 --kernel-trace --stats -d DIR -o convbn --output-format csv -- python tools/bench_convbn_train.py trace
    python tools/bench_convbn_train.py digest OUT.json DIR/.../convbn_kernel_stats.csv

``run`` times whole iterations with device events, the two sides alternating in one process (WARMUP iterations
each first), and reports the median and the spread per stack, the floor of the stack's products at the measured
fp32 MFMA rate of 155 TFLOP/s and the fraction of it reached; it also evaluates the bound of convbn_train_util.py
on the test cases (fixture masks, float64 restatement) and at the two bench shapes.  There every block is judged on
its own: the restatement is fed the block's input, upstream gradient and mask as the device run saw them, and the
number of kept relu elements within 1e-5 of the kink is recorded next to the figures (such an element may sit on the
other side of the kink in float32; the test cases have none).  ``trace`` runs TRACE_ITERS iterations of the device
path of both stacks for the kernel trace; ``digest`` adds each kernel's time per iteration from the trace's
statistics.  OUT.json's other sections are kept.  (profiles/convbn_train_kernel_stats.csv is that trace's file.)
"""
import csv
import importlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
PKG = "your-voice-tts_amd"
WARMUP, REPS, TRACE_ITERS = 5, 30, 10
MFMA_FP32_TFLOPS = 155.0


def _setup(name):
    import numpy as np
    import torch
    from torch import nn
    import convbn_train_util as cu
    layers = importlib.import_module(PKG + ".layers")
    inp = cu.inputs(cu.BENCH[name])
    ours, theirs = [], []
    for blk in inp["blocks"]:
        state = {k: torch.from_numpy(np.asarray(v)) for k, v in cu.state_dict(blk).items()}
        m = layers.ConvBNBlock(blk["cin"], blk["cout"], 5, blk["act"])
        m.load_state_dict(state)
        ours.append(m.cuda().train())
        act = {"relu": [nn.ReLU()], "tanh": [nn.Tanh()], None: []}[blk["act"]]
        t = nn.Module()
        t.net = nn.Sequential(nn.Conv1d(blk["cin"], blk["cout"], 5, padding=2), nn.BatchNorm1d(blk["cout"]), *act,
                              nn.Dropout(p=0.5))
        t.load_state_dict(state)
        theirs.append(t.cuda().train())
    x = torch.from_numpy(inp["x"]).cuda().requires_grad_(True)
    up = torch.from_numpy(inp["up"]).cuda()

    def device_path():
        h = x
        for m in ours:
            h = m(h)
        return [h] + list(torch.autograd.grad([h], [x] + [p for m in ours for p in m._params()], [up]))

    def torch_path():
        h = x
        for t in theirs:
            h = t.net(h)
        return [h] + list(torch.autograd.grad([h], [x] + [p for t in theirs for p in t.parameters()], [up]))

    return cu, inp, ours, x, up, device_path, torch_path


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def _stats(ts):
    ts = sorted(ts)
    return dict(ms_median=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1], ms_spread=ts[-1] - ts[0], reps=len(ts))


def _block_errors(cu, ours, x, up):
    """Every block of a stack against the restatement of that block alone, on what the device run saw."""
    import numpy as np
    import torch
    seen, h = [], x
    before = [(m.net[1].running_mean.cpu().numpy().astype(np.float64),
               m.net[1].running_var.cpu().numpy().astype(np.float64)) for m in ours]
    for m in ours:
        rec = dict(x=h.detach())
        h = m(h)
        rec["out"] = h.detach()
        h.register_hook(lambda g, rec=rec: rec.__setitem__("grad_out", g.detach()))
        seen.append(rec)
    grads = torch.autograd.grad([h], [x] + [p for m in ours for p in m._params()], [up])
    errors, near = {}, 0
    for i, (m, rec) in enumerate(zip(ours, seen)):
        blk = dict(act=m.nonlinear, cin=m.in_channels, cout=m.out_channels,
                   **{p: t.detach().cpu().numpy() for p, t in zip(cu.PARAMS, m._params())})
        mask = m.last_mask.cpu().numpy()
        out, saved, rm, rv = cu.block_forward(rec["x"].cpu().numpy().astype(np.float64), blk, mask, *before[i])
        gx, g, S = cu.block_backward(rec["grad_out"].cpu().numpy().astype(np.float64), blk, saved)
        got_gx = grads[0] if i == 0 else seen[i - 1]["grad_out"]
        e = {"out": cu.ratio(rec["out"].cpu().numpy(), out), "grad_x": cu.ratio(got_gx.cpu().numpy(), gx),
             "running_mean": cu.ratio(m.net[1].running_mean.cpu().numpy(), rm),
             "running_var": cu.ratio(m.net[1].running_var.cpu().numpy(), rv)}
        for j, p in enumerate(cu.PARAMS):
            e["grad_" + p] = cu.ratio(grads[1 + 4 * i + j].cpu().numpy(), g[p], S if p == "bias" else None)
        if m.nonlinear == "relu":
            e["kept_relu_elements_within_1e-5_of_the_kink"] = int(((np.abs(saved["z"]) < cu.MIN_Z) & (mask != 0)).sum())
            near += e["kept_relu_elements_within_1e-5_of_the_kink"]
        errors[f"block{i}"] = e
        print(f"block {i}: {e}", flush=True)
    return errors, near


def run(out_path):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: nothing to measure")
    layers = importlib.import_module(PKG + ".layers")
    timing, bench_errors = {}, {}
    for name in ("encoder", "postnet"):
        cu, inp, ours, x, up, device_path, torch_path = _setup(name)
        sides = {"layers.ConvBNBlock": device_path, "torch.nn.Sequential": torch_path}
        times = {k: [] for k in sides}
        for i in range(WARMUP + REPS):
            for side, fn in sides.items():  # alternating: both see the same machine state
                t, _ = _timed(fn)
                if i >= WARMUP:
                    times[side].append(t)
        it = {k: _stats(v) for k, v in times.items()}
        B, T = x.shape[0], x.shape[2]
        flops = sum(3 * 2 * B * T * b["cin"] * b["cout"] * 5 for b in inp["blocks"])
        floor_ms = flops / (MFMA_FP32_TFLOPS * 1e12) * 1e3
        ours_ms, torch_ms = it["layers.ConvBNBlock"]["ms_median"], it["torch.nn.Sequential"]["ms_median"]
        timing[name] = dict(
            shape=dict(B=B, T=T, blocks=[[b["cin"], b["cout"], b["act"]] for b in inp["blocks"]]), iterations=it,
            ratio_device_over_torch=ours_ms / torch_ms,
            device_below_torch_by_more_than_the_two_spreads=bool(
                torch_ms - ours_ms > it["layers.ConvBNBlock"]["ms_spread"] + it["torch.nn.Sequential"]["ms_spread"]),
            flops_forward_and_both_backward_products=flops, floor_ms_at_155_tflops=floor_ms,
            fraction_of_floor_reached=floor_ms / ours_ms)
        print(name, json.dumps(timing[name]), flush=True)
        bench_errors[name], near = _block_errors(cu, ours, x, up)
        bench_errors[name]["kept_relu_elements_within_1e-5_of_the_kink"] = near
        del ours, x, up, device_path, torch_path
        torch.cuda.empty_cache()

    # the bound on the test cases, against the float64 restatement, with the fixture's masks
    fixture = np.load(os.path.join(REPO, "tests", "golden", "convbn_train.npz"))
    errors = {}
    for case in cu.CASES:
        ci, masks = cu.inputs(case), cu.masks(fixture, case)
        blocks = []
        for blk in ci["blocks"]:
            m = layers.ConvBNBlock(blk["cin"], blk["cout"], 5, blk["act"])
            m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cu.state_dict(blk).items()})
            blocks.append(m.cuda().train())
        cx = torch.from_numpy(ci["x"]).cuda().requires_grad_(True)

        def fwd(h):
            for m, mask in zip(blocks, masks):
                h = m(h, torch.from_numpy(mask).cuda())
            return h

        o = fwd(cx)
        g = torch.autograd.grad([o], [cx] + [p for m in blocks for p in m._params()], [torch.from_numpy(ci["up"]).cuda()])
        r = {"out": o, "grad_x": g[0]}
        for i, m in enumerate(blocks):
            r.update({f"grad_{p}{i}": g[1 + 4 * i + j] for j, p in enumerate(cu.PARAMS)})
            r[f"rm1_{i}"], r[f"rv1_{i}"] = m.net[1].running_mean.clone(), m.net[1].running_var.clone()
        fwd(cx.detach())
        for i, m in enumerate(blocks):
            r[f"rm2_{i}"], r[f"rv2_{i}"] = m.net[1].running_mean.clone(), m.net[1].running_var.clone()
        ref = cu.restate(ci, masks)
        errors[case] = {k: cu.ratio(v.detach().cpu().numpy(), ref[k], cu.bias_scale(k, ref)) for k, v in r.items()}
    worst = max(max(v.values()) for v in errors.values())
    figures = lambda e: [v for b in e.values() if isinstance(b, dict) for k, v in b.items() if not k.startswith("kept")]

    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = dict(
        device=torch.cuda.get_device_name(0),
        what="forward + backward (out, grad_x, four parameter gradients per block) of a whole stack, device events "
             "around whole iterations, the two sides alternating in one process; ms_spread = max - min",
        warmup=WARMUP, stacks=timing)
    doc["device_errors"] = dict(
        what="the bound's figure of layers.ConvBNBlock against the float64 restatement (bound 4e-6; the conv bias "
             "gradient in the S form); at the bench shapes every block on its own, fed what the device run saw",
        worst_over_test_cases=worst, per_case=errors,
        worst_at_bench_shapes={k: max(figures(v)) for k, v in bench_errors.items()}, bench_shapes=bench_errors)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(dict(worst_device_error_over_test_cases=worst,
                          worst_at_bench_shapes=doc["device_errors"]["worst_at_bench_shapes"],
                          ratio_device_over_torch={k: v["ratio_device_over_torch"] for k, v in timing.items()})))
    assert worst <= cu.TOL, worst


def trace():
    import torch
    for name in ("encoder", "postnet"):
        device_path = _setup(name)[5]
        for _ in range(TRACE_ITERS):
            device_path()
        torch.cuda.synchronize()


def digest(out_path, stats_csv):
    doc = json.load(open(out_path))
    kernels, total = {}, 0
    for row in csv.DictReader(open(stats_csv)):
        name, calls, ns = row["Name"], int(row["Calls"]), int(float(row["TotalDurationNs"]))
        found = re.search(r"\bcb_[a-z0-9_]+_kernel\b", name)  # the kernels of csrc/convbn_train.hip
        if not found:
            continue
        short = found.group(0)
        kernels[short] = dict(calls_per_iteration=calls / TRACE_ITERS, us_per_iteration=ns / TRACE_ITERS / 1e3,
                              us_per_call=ns / calls / 1e3)
        total += ns
    for k in kernels.values():
        k["share"] = k["us_per_iteration"] * 1e3 * TRACE_ITERS / total
    doc["kernels"] = dict(what="rocprofv3 --kernel-trace --stats over %d iterations of the device path of both stacks "
                               "(an iteration = the encoder stack + the Postnet stack), in a run of its own"
                               % TRACE_ITERS, kernel_ms_per_iteration=total / TRACE_ITERS / 1e6, per_kernel=kernels)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc["kernels"]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "trace":
        trace()
    else:
        digest(sys.argv[2], sys.argv[3])
