"""The measurement behind profiles/decoder_train.json (DESIGN "Trainable decoder"): forward plus all gradients of the
teacher-forced decoder at the training shape B = 32, text lengths seeded in 40..150, T = 400 steps, r = 1, sigmoid
norm with forward attention, separate stopnet (tests/decoder_train_util.py: BENCH), as (a) layers.Decoder
(tts_dectrain_forward / tts_dectrain_backward) and (b) what train_batch ran before it: the same decoder in torch
ops, one step at a time (decoder_train_util.TorchDecoder), on the same device with the same weights, data and
dropout masks.  Both produce the outputs, grad_inputs, grad_memories and every parameter gradient.

    python tools/bench_decoder_train.py run OUT.json [REPS [WARMUP]]
    rocprofv3 --kernel-trace --stats -d DIR -o dec --output-format csv -- python tools/bench_decoder_train.py trace
    python tools/bench_decoder_train.py digest OUT.json DIR/.../dec_kernel_stats.csv
    python tools/bench_decoder_train.py errors OUT.json      (the bound's figure of every test case on the device)

``run`` times whole iterations with device events, the two sides alternating in one process (WARMUP iterations each
first, 2 by default, then REPS, 10 by default), and reports the medians, the ranges, the ratio and the device
path's time per step against the ~8 us it takes to stream a step's 71 MB of weights once at 8.6 TB/s.  ``trace``
runs TRACE_ITERS iterations of the device path alone for the kernel trace; ``digest`` adds each kernel's time per
iteration from the trace's statistics.  OUT.json's other sections are kept.
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
WARMUP, REPS, TRACE_ITERS = 2, 10, 3
FLOOR_US = 8.0


def _setup():
    import torch
    import decoder_train_util as du
    layers = importlib.import_module(PKG + ".layers")
    c = du.BENCH
    inp = du._draw(c, 0)  # (no kink search at this size: nothing here is compared across the kink)

    class Model(torch.nn.Module):
        pass

    theirs = du.torch_decoder(c, inp["weights"]).cuda().train()
    holder = Model()
    holder.decoder = du.torch_decoder(c, inp["weights"]).cuda().train()
    ours = layers.use_device_decoder(holder).decoder
    x = torch.from_numpy(inp["inputs"]).cuda().requires_grad_(True)
    mem = torch.from_numpy(inp["memories"]).cuda().requires_grad_(True)
    mask = torch.from_numpy(inp["mask"]).cuda()
    masks = {k: torch.from_numpy(v).cuda() for k, v in inp["masks"].items()}
    up_o, up_s = torch.from_numpy(inp["up"]["outputs"]).cuda(), torch.from_numpy(inp["up"]["stop_tokens"]).cuda()

    def path(dec):
        def fn():
            o, s, a = dec(x, mem, mask, masks)
            return [o, s, a] + list(torch.autograd.grad([o, s], [x, mem] + list(dec.parameters()), [up_o, up_s]))
        return fn

    return du, c, inp, ours, theirs, path(ours), path(theirs)


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


def run(out_path, reps=REPS, warmup=WARMUP):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: nothing to measure")
    du, c, inp, ours, theirs, device_path, torch_path = _setup()
    sides = {"layers.Decoder": device_path, "TorchDecoder": torch_path}
    times = {k: [] for k in sides}
    last = {}
    for i in range(warmup + reps):
        for name, fn in sides.items():  # alternating: both see the same machine state
            t, last[name] = _timed(fn)
            if i >= warmup:
                times[name].append(t)
            print(f"iteration {i} {name}: {t:.1f} ms", flush=True)
    timing = {k: _stats(v) for k, v in times.items()}
    ratio = timing["layers.Decoder"]["ms_median"] / timing["TorchDecoder"]["ms_median"]
    # the two sides against each other at this shape, in the bound's form (torch on the device is no reference:
    # this is a figure, not a check)
    names = ["outputs", "stop_tokens", "alignments", "grad_inputs", "grad_memories"] + ["grad_" + n for n, _ in ours.named_parameters()]
    between = {n: du.ratio(a.detach().cpu().numpy(), b.detach().cpu().numpy())
               for n, a, b in zip(names, last["layers.Decoder"], last["TorchDecoder"])}
    # forward and backward of the device path apart
    fwd = [_timed(lambda: ours(x_, m_, k_, s_))[0] for x_, m_, k_, s_ in [_args(inp)] * (warmup + reps)][warmup:]
    T, B = c["T"], len(c["lens"])
    dev = timing["layers.Decoder"]["ms_median"]
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["timing"] = dict(
        device=torch.cuda.get_device_name(0),
        shape=dict(B=B, T=T, r=c["r"], L=max(c["lens"]), lens=c["lens"], norm=c["norm"], forward_attn=c["fwd"],
                   separate_stopnet=c["sep"]),
        what="forward + every gradient, device events around whole iterations, the two sides alternating in one process",
        warmup=warmup, iterations=timing, ratio_device_over_torch=ratio,
        device_forward_only=_stats(fwd),
        per_step_us=dict(device_forward_plus_backward=dev * 1e3 / T, forward_only=_stats(fwd)["ms_median"] * 1e3 / T,
                         weight_streaming_floor_forward=FLOOR_US, weight_streaming_floor_backward=FLOOR_US),
        device_against_torch_at_this_shape=between)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(dict(iterations=timing, ratio_device_over_torch=ratio, per_step_us=doc["timing"]["per_step_us"],
                          worst_between=max(between.values()))))


def _args(inp):
    import torch
    return (torch.from_numpy(inp["inputs"]).cuda(), torch.from_numpy(inp["memories"]).cuda(),
            torch.from_numpy(inp["mask"]).cuda(), {k: torch.from_numpy(v).cuda() for k, v in inp["masks"].items()})


def errors(out_path):
    """The bound's figure of every test case on the device, against the float64 restatement."""
    import torch
    import decoder_train_util as du
    layers = importlib.import_module(PKG + ".layers")
    res = {}
    for case, c in du.CASES.items():
        inp, ref, d = du.inputs(case), du.restated(case), c["dims"]
        m = layers.Decoder(d["E"], d["mel"], c["r"], False, c["norm"], "original", c["pdrop"], c["fwd"], False, False, False,
                           c["sep"], prenet_dim=d["PN"], rnn_dim=d["R"], attention_dim=d["A"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
        m = m.cuda().train(c["training"])
        x = torch.from_numpy(inp["inputs"]).cuda().requires_grad_(c["training"])
        mem = torch.from_numpy(inp["memories"]).cuda().requires_grad_(c["training"])
        masks = None if inp["masks"] is None else {k: torch.from_numpy(v).cuda() for k, v in inp["masks"].items()}
        o, s, a = m(x, mem, torch.from_numpy(inp["mask"]).cuda(), masks)
        got = {"outputs": o, "stop_tokens": s, "alignments": a}
        if c["training"]:
            ((o * torch.from_numpy(inp["up"]["outputs"]).cuda()).sum()
             + (s * torch.from_numpy(inp["up"]["stop_tokens"]).cuda()).sum()).backward()
            got.update(grad_inputs=x.grad, grad_memories=mem.grad)
            got.update({"grad_" + n: p.grad for n, p in m.named_parameters()})
        res[case] = {n: du.ratio(got[n].detach().cpu().numpy(), ref[n], du.scale_of(case, n, ref))
                     for n in du.tensor_names(case)}
        print(case, max(res[case].values()), flush=True)
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["device_errors"] = dict(what="max|got - ref64| / max(1, scale) of layers.Decoder against the float64 restatement "
                                     "(bound 4e-6)", worst=max(max(v.values()) for v in res.values()), per_case=res)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)


def trace():
    import torch
    device_path = _setup()[5]
    for _ in range(TRACE_ITERS):
        device_path()
    torch.cuda.synchronize()


def digest(out_path, stats_csv):
    doc = json.load(open(out_path))
    kernels, total = {}, 0
    for row in csv.DictReader(open(stats_csv)):
        name, calls, ns = row["Name"], int(row["Calls"]), int(float(row["TotalDurationNs"]))
        found = re.search(r"\bdt_[a-z0-9_]+_kernel\b", name)  # the kernels of csrc/decoder_train.hip
        if not found:
            continue
        short = found.group(0)
        if "dt_step_kernel" in short:
            epi = re.search(r"dt_step_kernel<\s*(\d+)\s*,\s*(\d+)", name)
            short += "<%s>" % ("plain", "lstm_fwd", "lstm_bwd")[int(epi.group(2))] if epi else ""
        k = kernels.setdefault(short, dict(calls=0, ns=0))
        k["calls"] += calls
        k["ns"] += ns
        total += ns
    per = {n: dict(calls_per_iteration=k["calls"] / TRACE_ITERS, us_per_iteration=k["ns"] / TRACE_ITERS / 1e3,
                   us_per_call=k["ns"] / k["calls"] / 1e3, share=k["ns"] / total) for n, k in kernels.items()}
    doc["kernels"] = dict(what="rocprofv3 --kernel-trace --stats over %d iterations of the device path, in a run of "
                               "its own" % TRACE_ITERS, kernel_ms_per_iteration=total / TRACE_ITERS / 1e6, per_kernel=per)
    json.dump(doc, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc["kernels"]))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], *[int(v) for v in sys.argv[3:5]])
    elif sys.argv[1] == "trace":
        trace()
    elif sys.argv[1] == "errors":
        errors(sys.argv[2])
    else:
        digest(sys.argv[2], sys.argv[3])
