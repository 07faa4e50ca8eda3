"""Decoder loop time per step of the resident batch decoder (csrc/resident_batch.hip) against the
multi-launch batch and serial batch-1 resident calls, at the Synthesizer's configuration (mask off,
runs to the cap) and synthesize.py's (mask on).  GPU box helper; prints one JSON line per case.

    python tools/resident_batch_bench.py [--cap 1000] [--batches 2,3,4,8,12]

--attn picks attention configurations instead (a comma list), among them the general form's (location features,
windowing, transition agent), and measures the three paths alternately: per alternation one run of
(a) the resident batch decoder, (b) B serial batch-1 resident calls, (c) the multi-launch step
(TTS_RESIDENT_BATCH=0); medians and min..max of the decoder loop time per batch step.

    python tools/resident_batch_bench.py --attn loc_softmax --cap 300 --batches 2,3,4,8
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
t2 = importlib.import_module("your-voice-tts_amd.tacotron2")
weights = importlib.import_module("your-voice-tts_amd.weights")

ATTN = {
    "mask": dict(attn_norm="sigmoid", forward_attn=True, forward_attn_mask=True, location_attn=False),
    "nomask": dict(attn_norm="sigmoid", forward_attn=True, forward_attn_mask=False, location_attn=False),
    # the constructor default (models/tacotron2.py:17,23)
    "loc_softmax": dict(attn_norm="softmax", forward_attn=False, forward_attn_mask=False, location_attn=True),
    "loc_fwd_ta": dict(attn_norm="sigmoid", forward_attn=True, trans_agent=True, forward_attn_mask=False,
                       location_attn=True),
    "win_softmax": dict(attn_norm="softmax", forward_attn=False, forward_attn_mask=False, location_attn=False,
                        attn_win=True),
}


def model(attn, batch, cap):
    os.environ["TTS_RESIDENT_BATCH"] = "1" if batch else "0"
    m = t2.Tacotron2(130, 0, r=1, max_batch=16, max_len=256, **ATTN[attn])
    m.decoder.max_decoder_steps = cap
    m = m.cuda().eval()
    m.inference_batch([[5, 6], [7, 8, 9]])
    return m


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def loop_ms(m, ids):
    """Decoder loop time (device events) and steps of one inference_batch call."""
    out = m.inference_batch(ids)
    return m.last_timing.get("decoder_loop_ms"), max(out["steps"]), m.last_timing.get("resident_kind")


def alternate(attn, args):
    """One JSON line per batch: us per batch step of the three paths, medians over alternations."""
    rb, ml = model(attn, True, args.cap), model(attn, False, args.cap)
    for B in [int(x) for x in args.batches.split(",")]:
        ids = [weights.synthetic_ids(args.L, 1 + b) for b in range(B)]
        for m in (rb, ml):  # warm
            m.inference_batch(ids)
        rb.inference_batch(ids[:1])
        us = dict(resident_batch=[], serial_b1=[], multi_launch=[])
        kinds = {}
        for _ in range(args.alternations):
            ms, steps, kinds["resident_batch"] = loop_ms(rb, ids)
            us["resident_batch"].append(1000 * ms / steps)
            tot, smax = 0.0, 0
            for x in ids:
                ms, st, kinds["serial_b1"] = loop_ms(rb, [x])
                tot, smax = tot + ms, max(smax, st)
            us["serial_b1"].append(1000 * tot / smax)
            ms, st, kinds["multi_launch"] = loop_ms(ml, ids)
            us["multi_launch"].append(1000 * ms / st)
        rec = dict(attn=attn, B=B, L=args.L, cap=args.cap, steps=steps, alternations=args.alternations,
                   resident_kind=kinds)
        for k, v in us.items():
            rec[k + "_us_per_step"] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3),
                                           max=round(max(v), 3))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=1000)
    ap.add_argument("--batches", default="2,3,4,8,12")
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--mask", choices=("both", "on", "off"), default="both")
    ap.add_argument("--attn", help="attention configurations (comma list of %s), the three paths alternating"
                    % ", ".join(sorted(ATTN)))
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the resident batch decoder only")
    args = ap.parse_args()
    if args.attn:
        names = args.attn.split(",")
        if any(n not in ATTN for n in names):
            ap.error("--attn: one of " + ", ".join(sorted(ATTN)))
        for n in names:
            alternate(n, args)
        return
    for mask in {"both": (False, True), "on": (True,), "off": (False,)}[args.mask]:
        rb = model("mask" if mask else "nomask", True, args.cap)
        ml = None if args.quick else model("mask" if mask else "nomask", False, args.cap)
        for B in [int(x) for x in args.batches.split(",")]:
            ids = [weights.synthetic_ids(args.L, 1 + b) for b in range(B)]
            rec = dict(mask=mask, B=B, L=args.L, cap=args.cap)
            rec["resident_batch_ms"] = timed(lambda: rb.inference_batch(ids))
            rec["resident_kind"] = rb.last_timing.get("resident_kind")
            rec["decoder_loop_ms"] = rb.last_timing.get("decoder_loop_ms")
            steps = max(rb.inference_batch(ids)["steps"])
            rec["steps"] = steps
            rec["us_per_step"] = 1000 * rec["decoder_loop_ms"] / steps if steps else None
            if ml is not None:
                rec["multi_launch_ms"] = timed(lambda: ml.inference_batch(ids))
                rec["multi_launch_loop_ms"] = ml.last_timing.get("decoder_loop_ms")
                rec["serial_b1_ms"] = timed(lambda: [rb.inference_batch([x]) for x in ids], reps=1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
