"""The measurement behind profiles/eval_loss.json (DESIGN "Evaluation losses"): the masked L1 criterion at
B = 32, T = 800, D = 1025, lengths uniform in 300..800 (seed 0), as (a) losses.L1LossMasked (tts_loss_masked)
and (b) the reference's expression (layers/losses.py:27-32) written with PyTorch-ROCm ops on the same
device.  Four operand sets are used in turn (840 MB in all), so no call finds its operands in the 256 MiB
Infinity Cache.  One GPU process; meant to run once under the kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -o eval_loss --output-format csv -- python tools/eval_loss_bench.py run OUT.json
    python tools/eval_loss_bench.py digest OUT.json DIR/.../eval_loss_kernel_stats.csv profiles/eval_loss.json

``run`` times every call with device events (launches, the small copies and the host wait included) and
checks both values against each other; ``digest`` adds the kernels' own durations from the trace's
statistics (time per call = total kernel time / calls) and the achieved fraction of HBM bandwidth.
"""
import csv
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "your-voice-tts_amd"
B, T, D, SETS, WARMUP, REPS = 32, 800, 1025, 4, 4, 20
HBM_PEAK_TBS = 8.0  # MI355X HBM3E


def run(out):
    import numpy as np
    import torch
    from torch.nn import functional
    losses = importlib.import_module(PKG + ".losses")
    gu = importlib.import_module(PKG + ".generic_utils")
    lengths = np.random.Generator(np.random.PCG64(0)).integers(300, 801, B)
    g = torch.Generator().manual_seed(0)  # drawn on the host: the trace holds the two workloads' kernels only
    sets = [(torch.randn(B, T, D, generator=g).cuda(), torch.randn(B, T, D, generator=g).cuda()) for _ in range(SETS)]
    len_host, len_dev = torch.from_numpy(lengths), torch.from_numpy(lengths).cuda()
    crit = losses.L1LossMasked()

    def ours(x, y):
        return crit(x, y, len_host)

    def torch_expr(x, y):  # layers/losses.py:27-32
        mask = gu.sequence_mask(sequence_length=len_dev, max_len=y.size(1)).unsqueeze(2).float()
        mask = mask.expand_as(x)
        return functional.l1_loss(x * mask, y * mask, reduction="sum") / mask.sum()

    res = dict(device=torch.cuda.get_device_name(0), B=B, T=T, D=D, lengths=[int(v) for v in lengths],
               operand_sets=SETS, warmup=WARMUP, reps=REPS,
               bytes_owed=int(8 * D * np.minimum(lengths, T).sum()), bytes_padded_operands=8 * B * T * D)
    values = {}
    for name, fn in (("tts_loss_masked", ours), ("torch_expression", torch_expr)):
        ts = []
        for i in range(WARMUP + REPS):
            x, y = sets[i % SETS]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            v = fn(x, y)
            b.record()
            b.synchronize()
            if i >= WARMUP:
                ts.append(a.elapsed_time(b))
            values.setdefault(name, []).append(float(v))
        ts = sorted(ts)
        res[name] = dict(event_ms_median=ts[len(ts) // 2], event_ms_min=ts[0], event_ms_max=ts[-1],
                         calls=WARMUP + REPS, value_set0=values[name][0])
    rel = max(abs(a - b) / abs(b) for a, b in zip(values["tts_loss_masked"], values["torch_expression"]))
    res["max_relative_difference_of_the_float32_values"] = rel
    assert rel < 1e-4, rel  # (the torch side is a float32 tree sum of up to 26 M terms)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "lengths"}))


def digest(run_json, stats_csv, out):
    res = json.load(open(run_json))
    ours = dict(kernels={}, ns=0)
    other = dict(kernels={}, ns=0)
    copies = dict(kernels={}, ns=0)  # the runtime's copy / fill kernels: both workloads' small transfers
    for row in csv.DictReader(open(stats_csv)):
        name, calls, ns = row["Name"], int(row["Calls"]), int(float(row["TotalDurationNs"]))
        side = (ours if "loss_partial_kernel" in name or "loss_fold_kernel" in name
                else copies if name.startswith("__amd_rocclr_") else other)
        side["kernels"][name[:120]] = dict(calls=calls, total_ns=ns)
        side["ns"] += ns
    for key, side in (("tts_loss_masked", ours), ("torch_expression", other)):
        calls = res[key]["calls"]
        ms = side["ns"] / calls / 1e6
        res[key].update(kernel_ms_per_call=ms, kernels=side["kernels"],
                        owed_bytes_per_s_TB=res["bytes_owed"] / (ms * 1e-3) / 1e12,
                        fraction_of_hbm_peak=res["bytes_owed"] / (ms * 1e-3) / 1e12 / HBM_PEAK_TBS)
    res["hbm_peak_TBs"] = HBM_PEAK_TBS
    res["runtime_copy_kernels"] = copies["kernels"]
    res["note"] = ("torch_expression's kernels are every kernel of the trace that is neither a loss kernel nor one "
                   "of the runtime's copy / fill kernels (listed apart: they serve both workloads)")
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in res[k].items() if kk != "kernels"}
                      for k in ("tts_loss_masked", "torch_expression")}))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        digest(*sys.argv[2:5])
