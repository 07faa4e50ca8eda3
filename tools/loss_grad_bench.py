"""The measurement behind profiles/loss_grad.json (DESIGN "Loss gradients"): forward plus backward of the three
training criteria of a Tacotron2 iteration (train.py:139-157: MSELossMasked on the decoder and the postnet
output, BCEWithLogitsLoss on the stop logits) at B = 32, T = 800, D = 80, lengths uniform in 300..800 (seed 0),
as (a) the package's criteria (tts_loss_masked, tts_loss_bce_logits, tts_loss_backward) and (b) the reference's
expressions (layers/losses.py:56-61, nn.BCEWithLogitsLoss) written with PyTorch-ROCm ops and autograd on the
same device.  The tensors are a few MB: they stay in the caches, and launches, not bandwidth, are what is timed.
One GPU process; ``run`` once with the profiler off, once more under the kernel trace for the kernels' own times:

    python tools/loss_grad_bench.py run OUT.json
    rocprofv3 --kernel-trace --stats -d DIR -o loss_grad --output-format csv -- python tools/loss_grad_bench.py run TRACED.json
    python tools/loss_grad_bench.py digest OUT.json DIR/.../loss_grad_kernel_stats.csv profiles/loss_grad.json

``run`` times every forward-plus-backward with device events (launches, the small copies and the forward's host
wait included), the two workloads in turn, and checks the values and the gradients against each other; ``digest``
adds the gradient kernel's own duration from the trace's statistics and the bytes per second it achieved over
the bytes it owes: 12 per valid element (two reads, one write) and 4 per padding element.
"""
import csv
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "your-voice-tts_amd"
B, T, D, WARMUP, REPS = 32, 800, 80, 10, 100
HBM_PEAK_TBS = 8.0  # MI355X HBM3E


def run(out):
    import numpy as np
    import torch
    from torch.nn import functional
    losses = importlib.import_module(PKG + ".losses")
    gu = importlib.import_module(PKG + ".generic_utils")
    lengths = np.random.Generator(np.random.PCG64(0)).integers(300, 801, B)
    g = torch.Generator().manual_seed(0)  # drawn on the host: a trace holds the two workloads' kernels only
    dec, post = (torch.randn(B, T, D, generator=g).cuda().requires_grad_() for _ in range(2))
    mel = torch.randn(B, T, D, generator=g).cuda()
    stop = (3.0 * torch.randn(B, T, generator=g)).cuda().requires_grad_()
    stop_targets = (torch.arange(T)[None, :] >= torch.from_numpy(lengths)[:, None] - 1).float().cuda()
    len_host, len_dev = torch.from_numpy(lengths), torch.from_numpy(lengths).cuda()
    criterion, criterion_st = losses.MSELossMasked(), losses.BCEWithLogitsLoss()

    def ours():
        return criterion(dec, mel, len_host) + criterion(post, mel, len_host) + criterion_st(stop, stop_targets)

    def masked(x, y):  # layers/losses.py:56-61
        mask = gu.sequence_mask(sequence_length=len_dev, max_len=y.size(1)).unsqueeze(2).float()
        mask = mask.expand_as(x)
        return functional.mse_loss(x * mask, y * mask, reduction="sum") / mask.sum()

    def torch_expr():
        return masked(dec, mel) + masked(post, mel) + functional.binary_cross_entropy_with_logits(stop, stop_targets)

    valid = int(D * np.minimum(lengths, T).sum())
    owed = dict(masked=12 * valid + 4 * (B * T * D - valid), bce=12 * B * T)
    res = dict(device=torch.cuda.get_device_name(0), B=B, T=T, D=D, lengths=[int(v) for v in lengths], warmup=WARMUP,
               reps=REPS, backward_bytes_owed_per_launch=owed, backward_bytes_owed=2 * owed["masked"] + owed["bce"],
               backward_launches_per_iteration=3)
    times = {"device_criteria": [], "torch_expression": []}
    kept = {}
    for i in range(WARMUP + REPS):
        for name, fn in (("device_criteria", ours), ("torch_expression", torch_expr)):
            dec.grad = post.grad = stop.grad = None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = fn()
            loss.backward()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                times[name].append(a.elapsed_time(b))
            kept[name] = (float(loss.detach()), dec.grad, post.grad, stop.grad)
    for name, ts in times.items():
        ts = sorted(ts)
        res[name] = dict(event_ms_median=ts[len(ts) // 2], event_ms_min=ts[0], event_ms_max=ts[-1],
                         iterations=WARMUP + REPS, loss=kept[name][0])
    ours_, theirs = kept["device_criteria"], kept["torch_expression"]
    res["relative_difference_of_the_loss"] = abs(ours_[0] - theirs[0]) / abs(theirs[0])
    res["max_gradient_difference_over_max_gradient"] = max(
        float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours_[1:], theirs[1:]))
    assert res["relative_difference_of_the_loss"] < 1e-4 and res["max_gradient_difference_over_max_gradient"] < 1e-5, res
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "lengths"}))


def digest(run_json, stats_csv, out):
    res = json.load(open(run_json))
    ours = {}
    for row in csv.DictReader(open(stats_csv)):
        name = row["Name"]
        if any(k in name for k in ("loss_grad_kernel", "loss_partial_kernel", "loss_fold_kernel")):
            ours[name[:120]] = dict(calls=int(row["Calls"]), total_ns=int(float(row["TotalDurationNs"])))
    grad = {k: v for k, v in ours.items() if "loss_grad_kernel" in k}
    calls, ns = sum(v["calls"] for v in grad.values()), sum(v["total_ns"] for v in grad.values())
    iterations = calls / res["backward_launches_per_iteration"]
    us = ns / iterations / 1e3  # the three launches of one iteration
    res["backward_kernel"] = dict(launches=calls, us_per_iteration_of_three_launches=us, us_per_launch=ns / calls / 1e3,
                                  owed_bytes_per_s_TB=res["backward_bytes_owed"] / (us * 1e-6) / 1e12,
                                  fraction_of_hbm_peak=res["backward_bytes_owed"] / (us * 1e-6) / 1e12 / HBM_PEAK_TBS)
    for v in ours.values():
        v["us_per_launch"] = v["total_ns"] / v["calls"] / 1e3
    res["kernels_in_the_traced_run"] = ours
    res["hbm_peak_TBs"] = HBM_PEAK_TBS
    res["note"] = ("event times are from the run with the profiler off; the kernel durations are from a second, traced "
                   "run of the same command.  The operands (6.6 MB per masked criterion) fit the caches, so bytes per "
                   "second is a rate over owed bytes, not an HBM figure")
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("device_criteria", "torch_expression", "backward_kernel")}))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        digest(*sys.argv[2:5])
