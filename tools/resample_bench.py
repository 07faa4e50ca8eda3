"""The measurement behind profiles/resample.json (DESIGN "Resampling"): AudioProcessor.resample_batch
(tts_gl_resample) on B = 32 files of 10 s, first 48 000 -> 22 050 Hz (139 taps per wing), then
16 000 -> 22 050 Hz (64 taps per wing).  One GPU process per step:

    python tools/resample_bench.py run OUT.json
    rocprofv3 --kernel-trace --stats -d DIR -o down --output-format csv -- python tools/resample_bench.py trace down
    rocprofv3 --kernel-trace --stats -d DIR -o up --output-format csv -- python tools/resample_bench.py trace up
    python tools/resample_bench.py digest OUT.json DIR/.../down_kernel_stats.csv DIR/.../up_kernel_stats.csv profiles/resample.json

``run`` (profiler off) times every call with device events (the launch, the descriptor upload and the host
wait included), then runs the host restatement of tests/resample_util.py on the same batch, records its wall
time and checks every sample of the device result against it bitwise.  That restatement is an unoptimised
numpy comparator, the only one available here (librosa and resampy are not installed); it is no baseline to
beat by a stated factor.  ``trace`` runs one workload's calls alone for the kernel trace; ``digest`` adds the
kernel's own duration from the trace's statistics and the rates that follow from it.
"""
import csv
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
PKG = "your-voice-tts_amd"
B, SECONDS, TARGET, WARMUP, REPS = 32, 10, 22050, 2, 10
WORKLOADS = {"down": 48000, "up": 16000}


def batch(orig_sr):
    import numpy as np
    N = SECONDS * orig_sr
    t = np.arange(N)
    rows = [(0.5 * np.sin(2 * np.pi * (220 + 20 * b) * t / orig_sr) + 0.01 * np.random.RandomState(b).randn(N))
            .astype(np.float32) for b in range(B)]
    return rows, N


def processor():
    cfg = json.load(open(os.path.join(REPO, PKG, "configs", "config_tacotron2.json")))["audio"]
    return importlib.import_module(PKG + ".audio").AudioProcessor(**cfg)


def timed_calls(ap, wav, N, orig_sr):
    import torch
    ts, out = [], None
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out, n_fix = ap.resample_batch(wav, [N] * B, orig_sr, TARGET)
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ts.append(a.elapsed_time(b))
    return sorted(ts), out, n_fix


def upload(rows):
    import numpy as np
    import torch
    return torch.from_numpy(np.stack(rows).astype(np.float64)).cuda()


def run(out):
    import numpy as np
    import torch
    import resample_util as ru
    ap = processor()
    res = dict(device=torch.cuda.get_device_name(0), B=B, seconds=SECONDS, target_sr=TARGET, warmup=WARMUP, reps=REPS)
    for name, orig_sr in WORKLOADS.items():
        rows, N = batch(orig_sr)
        ts, dev, n_fix = timed_calls(ap, upload(rows), N, orig_sr)
        n_res = ru.lengths(N, orig_sr, TARGET)[0]
        ratio = float(TARGET) / orig_sr
        step = int(min(1.0, ratio) * 512)
        taps = 32769 // step
        t0 = time.perf_counter()
        want = [ru.resample_ref(x, orig_sr, TARGET) for x in rows]
        host_s = time.perf_counter() - t0
        got = dev.cpu().numpy()
        differ = sum(int((ru.bits(got[b, :n_fix[b]]) != ru.bits(want[b])).sum()) for b in range(B))
        assert differ == 0, differ
        res[name] = dict(orig_sr=orig_sr, N=N, n_res=n_res, n_fix=n_fix[0], outputs=B * n_res, step=step,
                         taps_per_wing=taps, chain_steps_per_output=2 * taps,
                         table_gathers_per_output=2 * taps, bytes_in=8 * B * N, bytes_out=8 * B * n_fix[0],
                         event_ms_median=ts[len(ts) // 2], event_ms_min=ts[0], event_ms_max=ts[-1],
                         calls=WARMUP + REPS, samples_differing_from_the_restatement=differ,
                         numpy_comparator_wall_s=host_s)
    res["numpy_comparator"] = ("tests/resample_util.py resample_ref on one host thread: an unoptimised restatement, "
                               "the only comparator available; not a baseline to beat by a stated factor")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


def trace(name):
    ap = processor()
    rows, N = batch(WORKLOADS[name])
    ts, _, _ = timed_calls(ap, upload(rows), N, WORKLOADS[name])
    print(name, "event ms under the tracer", ts)


def digest(run_json, down_csv, up_csv, out):
    res = json.load(open(run_json))
    for name, path in (("down", down_csv), ("up", up_csv)):
        w = res[name]
        for row in csv.DictReader(open(path)):
            if "resample_kernel" in row["Name"]:
                calls, ns = int(row["Calls"]), int(float(row["TotalDurationNs"]))
                assert calls == w["calls"], (calls, w["calls"])
                ms = ns / calls / 1e6
                w.update(kernel_ms_per_call=ms, kernel_calls=calls, kernel_total_ns=ns,
                         output_samples_per_s=w["outputs"] / (ms * 1e-3),
                         taps_per_s=w["outputs"] * 2 * w["taps_per_wing"] / (ms * 1e-3),
                         owed_bytes_per_s_TB=(w["bytes_in"] + w["bytes_out"]) / (ms * 1e-3) / 1e12)
        assert "kernel_ms_per_call" in w, "no resample_kernel row in " + path
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "trace":
        trace(sys.argv[2])
    else:
        digest(*sys.argv[2:6])
