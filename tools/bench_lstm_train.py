"""The measurement behind profiles/lstm_train.json (DESIGN "Trainable LSTM"): forward + backward of the encoder's
LSTM at the training shape B = 32, I = 512, H = 256, bidirectional, lengths seeded and uniform in 40..150
(tests/lstm_train_util.py: BENCH), as (a) layers.LSTM (tts_lstm_forward / tts_lstm_backward) and (b) what
train_batch ran before it: torch.nn.LSTM on the device with pack_padded_sequence / pad_packed_sequence, on the
same data.  Both produce out and every gradient (grad_x and the eight parameter gradients).

    python tools/bench_lstm_train.py run OUT.json
    rocprofv3 --kernel-trace --stats -d DIR -o lstm --output-format csv -- python tools/bench_lstm_train.py trace
    python tools/bench_lstm_train.py digest OUT.json DIR/.../lstm_kernel_stats.csv

``run`` times whole iterations with device events, the two sides alternating in one process (WARMUP iterations
each first), and reports the median and the spread; it also times the device path's phases (a forward without
and with the reserve, a backward with no gradient asked for = the recurrence alone, and with each product
added) and evaluates the bound of lstm_train_util.py at this shape and on the test cases against the float64
restatement.  ``trace`` runs TRACE_ITERS iterations of the device path alone for the kernel trace; ``digest``
adds each kernel's time per iteration from the trace's statistics.  OUT.json's other sections are kept.
(profiles/lstm_train_kernel_stats.csv is that trace's statistics file.)
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


def _setup():
    import numpy as np
    import torch
    from torch import nn
    import lstm_train_util as lu
    layers = importlib.import_module(PKG + ".layers")
    inp = lu.inputs(lu.BENCH)
    state = {k: torch.from_numpy(v) for k, v in inp["weights"].items()}
    ours = layers.LSTM(inp["I"], inp["H"], batch_first=True, bidirectional=True)
    ours.load_state_dict(state)
    ours = ours.cuda().train()
    theirs = nn.LSTM(inp["I"], inp["H"], num_layers=1, batch_first=True, bidirectional=True)
    theirs.load_state_dict(state)
    theirs = theirs.cuda().train()
    x = torch.from_numpy(inp["x"]).cuda().requires_grad_(True)
    up = torch.from_numpy(inp["up"]).cuda()
    lens = inp["lens"]
    lens_np = np.asarray(lens)

    def device_path():
        out = ours.lstm(x, lens)[0]
        return [out] + list(torch.autograd.grad([out], [x] + list(ours.parameters()), [up]))

    def torch_path():  # Encoder.forward's calls (layers/tacotron2.py:68-75); the lengths are not sorted here
        packed = nn.utils.rnn.pack_padded_sequence(x, lens_np, batch_first=True, enforce_sorted=False)
        theirs.flatten_parameters()
        out = nn.utils.rnn.pad_packed_sequence(theirs(packed)[0], batch_first=True)[0]
        return [out] + list(torch.autograd.grad([out], [x] + list(theirs.parameters()), [up]))

    return lu, inp, ours, x, up, lens, device_path, torch_path


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
    import numpy as np
    import torch
    lu, inp, ours, x, up, lens, device_path, torch_path = _setup()
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: nothing to measure")
    sides = {"layers.LSTM": device_path, "torch.nn.LSTM": torch_path}
    times = {k: [] for k in sides}
    for i in range(WARMUP + REPS):
        for name, fn in sides.items():  # alternating: both see the same machine state
            t, _ = _timed(fn)
            if i >= WARMUP:
                times[name].append(t)
    timing = {k: _stats(v) for k, v in times.items()}
    ratio = timing["layers.LSTM"]["ms_median"] / timing["torch.nn.LSTM"]["ms_median"]

    # phases of the device path (whole calls, launches included)
    B, T = x.shape[0], x.shape[1]
    xd = x.detach()
    n = 2 * len(lu.PARAMS)
    fwd = lambda keep: ours._run_forward(xd, lens, None, None, keep)
    out, _, _, reserve = fwd(True)
    bwd = lambda need_x, need_p: ours._run_backward(xd, lens, reserve, out, None, up, need_x, need_p)
    only = lambda k: [i % 4 == k for i in range(n)]
    phases = {
        "forward_no_reserve": lambda: fwd(False), "forward_with_reserve": lambda: fwd(True),
        "backward_recurrence_only": lambda: bwd(False, [False] * n),
        "backward_plus_grad_x": lambda: bwd(True, [False] * n),
        "backward_plus_grad_w_ih": lambda: bwd(False, only(0)),
        "backward_plus_grad_w_hh": lambda: bwd(False, only(1)),
        "backward_plus_grad_biases": lambda: bwd(False, [i % 4 >= 2 for i in range(n)]),
        "backward_all": lambda: bwd(True, [True] * n),
    }
    phase_ms = {}
    for name, fn in phases.items():
        ts = [_timed(fn)[0] for _ in range(WARMUP + REPS)][WARMUP:]
        phase_ms[name] = _stats(ts)

    # the bound at this shape and on the test cases, against the float64 restatement
    names = lu.tensor_names(True)
    got = dict(zip(["out", "grad_x"] + ["grad_" + p for p in lu.param_names(True)], device_path()))
    got.update(zip(("h_n", "c_n"), ours.lstm(xd, lens)[1]))
    ref = lu.restate(inp)
    errors = {"bench_shape": {k: lu.ratio(got[k].detach().cpu().numpy(), ref[k]) for k in names}}
    theirs = dict(zip(["out", "grad_x"] + ["grad_" + p for p in lu.param_names(True)], torch_path()))
    torch_errors = {k: lu.ratio(theirs[k].detach().cpu().numpy(), ref[k]) for k in theirs}
    layers = importlib.import_module(PKG + ".layers")
    for case, c in lu.CASES.items():
        ci = lu.inputs(case)
        m = layers.LSTM(ci["I"], ci["H"], batch_first=True, bidirectional=ci["bi"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in ci["weights"].items()})
        m = m.cuda().train()
        cx = torch.from_numpy(ci["x"]).cuda().requires_grad_(True)
        hx = None if ci["h0"] is None else (torch.from_numpy(ci["h0"]).cuda(), torch.from_numpy(ci["c0"]).cuda())
        o, (h_n, c_n) = m.lstm(cx, ci["lens"], hx)
        g = torch.autograd.grad([o], [cx] + list(m.parameters()), [torch.from_numpy(ci["up"]).cuda()])
        r = dict(zip(["out", "h_n", "c_n", "grad_x"] + ["grad_" + p for p in lu.param_names(ci["bi"])],
                     (o, h_n, c_n) + tuple(g)))
        cref = lu.restate(ci)
        errors[case] = {k: lu.ratio(v.detach().cpu().numpy(), cref[k]) for k, v in r.items()}
    worst = max(max(v.values()) for v in errors.values())

    total = int(np.sum(lens))
    G, I, H = 4 * inp["H"], inp["I"], inp["H"]
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = dict(
        device=torch.cuda.get_device_name(0), shape=dict(B=B, Tmax=T, I=I, H=H, bidirectional=True, lens=lens,
                                                         valid_positions=total),
        what="forward + backward (out, grad_x, eight parameter gradients), device events around whole iterations, "
             "the two sides alternating in one process", warmup=WARMUP, iterations=timing,
        ratio_device_over_torch=ratio, device_path_phases=phase_ms,
        flops=dict(input_projection=2 * total * 2 * G * I, recurrence_forward=2 * total * 2 * G * H,
                   recurrence_backward=2 * total * 2 * G * H, grad_w_ih=2 * total * 2 * G * I,
                   grad_w_hh=2 * total * 2 * G * H, grad_x=2 * total * 2 * G * I))
    doc["device_errors"] = dict(what="max|got - ref64| / max(1, max|ref64|) of layers.LSTM against the float64 "
                                     "restatement (bound 4e-6)", worst=worst, per_case=errors,
                                torch_nn_lstm_on_the_device_at_bench_shape=torch_errors)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(dict(iterations=timing, ratio_device_over_torch=ratio, worst_device_error=worst,
                          phases={k: v["ms_median"] for k, v in phase_ms.items()})))
    assert worst <= lu.TOL, worst


def trace():
    import torch
    device_path = _setup()[6]
    for _ in range(TRACE_ITERS):
        device_path()
    torch.cuda.synchronize()


def digest(out_path, stats_csv):
    doc = json.load(open(out_path))
    kernels, total = {}, 0
    for row in csv.DictReader(open(stats_csv)):
        name, calls, ns = row["Name"], int(row["Calls"]), int(float(row["TotalDurationNs"]))
        found = re.search(r"\blt_[a-z_]+_kernel\b", name)  # the kernels of csrc/lstm_train.hip
        if not found:
            continue
        short = found.group(0)
        kernels[short] = dict(calls_per_iteration=calls / TRACE_ITERS, us_per_iteration=ns / TRACE_ITERS / 1e3,
                              us_per_call=ns / calls / 1e3)
        total += ns
    for k in kernels.values():
        k["share"] = k["us_per_iteration"] * 1e3 * TRACE_ITERS / total
    doc["kernels"] = dict(what="rocprofv3 --kernel-trace --stats over %d iterations of the device path, in a run of "
                               "its own" % TRACE_ITERS, kernel_ms_per_iteration=total / TRACE_ITERS / 1e6,
                          per_kernel=kernels)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc["kernels"]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "trace":
        trace()
    else:
        digest(sys.argv[2], sys.argv[3])
