"""The measurement behind profiles/gru_train.json (DESIGN "Trainable GRU"): forward + backward of the GRU at the
training shapes of its three sites in the reference's TacotronGST (tests/gru_train_util.py: BENCH),

    encoder   B 32, T 150, I 128, H 128, bidirectional, upstream gradient on out
    postnet   B 32, T 600, I 128, H 128, bidirectional, upstream gradient on out
    gst       B 32, T 10,  I 256, H 128, one direction, upstream gradient on h_n only

as (a) layers.GRU (tts_gru_forward / tts_gru_backward: the time loop inside one launch), (b) torch.nn.GRU on the
same device and data, and (c) a layers.GRU whose handle was created with TTS_GRU_STEPWISE=1: the same two recurrence
kernels launched once per time step.  All produce out, h_n and every gradient (grad_x and the parameter gradients).

    python tools/bench_gru_train.py run OUT.json
    rocprofv3 --kernel-trace --stats -d DIR -o gru --output-format csv -- python tools/bench_gru_train.py trace
    python tools/bench_gru_train.py digest OUT.json DIR/.../gru_kernel_stats.csv

``run`` times whole iterations with device events, the sides alternating in one process (WARMUP iterations each
first), and reports the median and the spread; it also times the device path's phases (whole calls) and evaluates
the bound of gru_train_util.py at these shapes and on the test cases against the float64 restatement
("device_errors").  ``trace`` runs TRACE_ITERS iterations of the device path at the encoder shape alone for the
kernel trace; ``digest`` adds each kernel's calls and time per iteration from the trace's statistics.  OUT.json's
other sections are kept.  (profiles/gru_train_kernel_stats.csv is that trace's statistics file.)
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
WARMUP, REPS, TRACE_ITERS = 5, 20, 10
STEPWISE = "TTS_GRU_STEPWISE"


def _setup(case):
    import torch
    from torch import nn
    import gru_train_util as gu
    layers = importlib.import_module(PKG + ".layers")
    inp = gu.inputs(case)
    state = {k: torch.from_numpy(v) for k, v in inp["weights"].items()}
    ours = layers.GRU(inp["I"], inp["H"], batch_first=True, bidirectional=inp["bi"])
    ours.load_state_dict(state)
    ours = ours.cuda().train()
    stepwise = layers.GRU(inp["I"], inp["H"], batch_first=True, bidirectional=inp["bi"])
    stepwise.load_state_dict(state)
    stepwise = stepwise.cuda().train()
    if torch.cuda.is_available():
        os.environ[STEPWISE] = "1"  # the library reads it when a handle is created
        try:
            stepwise._handle()
        finally:
            del os.environ[STEPWISE]
    theirs = nn.GRU(inp["I"], inp["H"], 1, batch_first=True, bidirectional=inp["bi"])
    theirs.load_state_dict(state)
    theirs = theirs.cuda().train()
    cuda = lambda a: None if a is None else torch.from_numpy(a).cuda()
    x = cuda(inp["x"]).requires_grad_(True)
    h0, up_out, up_hn = cuda(inp["h0"]), cuda(inp["up_out"]), cuda(inp["up_hn"])

    def path(module):
        def fn():
            module.flatten_parameters()
            out, h_n = module(x, h0)
            ups = [(t, u) for t, u in ((out, up_out), (h_n, up_hn)) if u is not None]
            return [out, h_n] + list(torch.autograd.grad([t for t, _ in ups], [x] + list(module.parameters()),
                                                         [u for _, u in ups]))
        return fn

    return gu, inp, ours, path(ours), path(theirs), stepwise, path(stepwise)


def _named(gu, inp, tensors):
    return dict(zip(["out", "h_n", "grad_x"] + ["grad_" + p for p in gu.param_names(inp["bi"])], tensors))


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
    return dict(ms_median=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1], reps=len(ts))


def run(out_path):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: nothing to measure")
    import gru_train_util as gu
    timing, errors, torch_errors = {}, {}, {}
    for site, case in gu.BENCH.items():
        _, inp, ours, device_path, torch_path, stepwise, stepwise_path = _setup(case)
        sides = {"layers.GRU": device_path, "torch.nn.GRU": torch_path, "layers.GRU stepwise": stepwise_path}
        times = {k: [] for k in sides}
        for i in range(WARMUP + REPS):
            for name, fn in sides.items():  # alternating: all see the same machine state
                t, _ = _timed(fn)
                if i >= WARMUP:
                    times[name].append(t)
        it = {k: _stats(v) for k, v in times.items()}
        # phases of the device path (whole calls, launches included)
        x = torch.from_numpy(inp["x"]).cuda()
        n = len(gu.param_names(inp["bi"]))
        cuda = lambda a: None if a is None else torch.from_numpy(a).cuda()
        up_out, up_hn = cuda(inp["up_out"]), cuda(inp["up_hn"])
        phases = {}
        for m, tag in ((ours, ""), (stepwise, "_stepwise")):
            fwd = lambda keep, m=m: m._run_forward(x, None, keep)
            out, _, reserve = fwd(True)
            bwd = lambda need_x, need_p, m=m, out=out, reserve=reserve: m._run_backward(x, reserve, out, None, up_out,
                                                                                         up_hn, need_x, need_p)
            phases.update({"forward_no_reserve" + tag: lambda fwd=fwd: fwd(False),
                           "forward_with_reserve" + tag: lambda fwd=fwd: fwd(True),
                           "backward_recurrence_only" + tag: lambda bwd=bwd: bwd(False, [False] * n),
                           "backward_all" + tag: lambda bwd=bwd: bwd(True, [True] * n)})
        phase_ms = {}
        for name, fn in phases.items():
            phase_ms[name] = _stats([_timed(fn)[0] for _ in range(WARMUP + REPS)][WARMUP:])
        c = gu._case(case)
        timing[site] = dict(shape={k: c[k] for k in ("B", "T", "I", "H", "bi")}, upstream=c.get("ups", "out"),
                            iterations=it, device_path_phases=phase_ms,
                            ratio_device_over_torch=it["layers.GRU"]["ms_median"] / it["torch.nn.GRU"]["ms_median"],
                            ratio_single_launch_over_stepwise=it["layers.GRU"]["ms_median"] /
                            it["layers.GRU stepwise"]["ms_median"])
        ref = gu.restate(inp)
        got, theirs, step = (_named(gu, inp, f()) for f in (device_path, torch_path, stepwise_path))
        errors["bench_" + site] = {k: gu.ratio(v.detach().cpu().numpy(), ref[k]) for k, v in got.items()}
        torch_errors[site] = {k: gu.ratio(v.detach().cpu().numpy(), ref[k]) for k, v in theirs.items()}
        assert all(torch.equal(got[k], step[k]) for k in got), "the stepwise launches give other bits"
    for case in gu.CASES:
        _, inp, _, device_path = _setup(case)[:4]
        ref = gu.restate(inp)
        errors[case] = {k: gu.ratio(v.detach().cpu().numpy(), ref[k]) for k, v in _named(gu, inp, device_path()).items()}
    worst = max(max(v.values()) for v in errors.values())

    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = dict(
        device=torch.cuda.get_device_name(0),
        what="forward + backward (out, h_n, grad_x, every parameter gradient), device events around whole "
             "iterations, the sides alternating in one process; 'stepwise' = the same recurrence kernels launched "
             "once per time step (TTS_GRU_STEPWISE=1), bitwise the same results", warmup=WARMUP, sites=timing)
    doc["device_errors"] = dict(what="max|got - ref64| / max(1, max|ref64|) of layers.GRU against the float64 "
                                     "restatement (bound 4e-6): the worst tensor per case", worst=worst,
                                per_case={k: max(v.values()) for k, v in errors.items()}, per_tensor=errors,
                                torch_nn_gru_on_the_device_at_bench_shapes=torch_errors)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(dict(worst_device_error=worst, sites={
        s: dict(ms={k: v["ms_median"] for k, v in t["iterations"].items()},
                phases={k: v["ms_median"] for k, v in t["device_path_phases"].items()}) for s, t in timing.items()})))
    assert worst <= gu.TOL, worst


def trace():
    import torch
    import gru_train_util as gu
    device_path = _setup(gu.BENCH["encoder"])[3]
    for _ in range(TRACE_ITERS):
        device_path()
    torch.cuda.synchronize()


def digest(out_path, stats_csv):
    doc = json.load(open(out_path))
    kernels, total = {}, 0
    for row in csv.DictReader(open(stats_csv)):
        name, calls, ns = row["Name"], int(row["Calls"]), int(float(row["TotalDurationNs"]))
        found = re.search(r"\bgt_[a-z_]+_kernel\b", name)  # the kernels of csrc/gru_train.hip
        if not found:
            continue
        short = found.group(0)
        kernels[short] = dict(calls_per_iteration=calls / TRACE_ITERS, us_per_iteration=ns / TRACE_ITERS / 1e3,
                              us_per_call=ns / calls / 1e3)
        total += ns
    for k in kernels.values():
        k["share"] = k["us_per_iteration"] * 1e3 * TRACE_ITERS / total
    doc["kernels"] = dict(what="rocprofv3 --kernel-trace --stats over %d iterations of the device path at the encoder "
                               "shape (one set_weights included), in a run of its own" % TRACE_ITERS,
                          kernel_ms_per_iteration=total / TRACE_ITERS / 1e6, per_kernel=kernels)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc["kernels"]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "trace":
        trace()
    else:
        digest(sys.argv[2], sys.argv[3])
