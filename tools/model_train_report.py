"""Whole-model gradient parity on the device, as a report: one training iteration of every case of
tests/model_train_util.py with the three device layers swapped in, every output, loss, gradient norm and parameter
gradient against the float64 twin and the reference's float64 run (tests/golden/model_train.npz) in the relative
bound's form.  Prints the worst figure per case and tensor against its bound and writes all of them into
profiles/model_train.json under "device_errors" (other sections are left as they are).  Needs an MI355X:

    python tools/model_train_report.py [--out profiles/model_train.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import model_train_util as mu  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "model_train.json"))
    args = ap.parse_args()
    layers, losses = (importlib.import_module("your-voice-tts_amd." + n) for n in ("layers", "losses"))
    gold = np.load(os.path.join(REPO, "tests", "golden", "model_train.npz"))
    per_case, failed = {}, []
    for case in mu.CASES:
        report = {}
        try:
            mu.compare(case, mu.device_iterate(case, layers, losses), mu.twin(case), gold, report)
        except AssertionError as e:
            failed.append(str(e))
        per_case[case] = {n: dict(figure=v, bound=tol) for n, (v, tol) in report.items()}
        name, (v, tol) = max(report.items(), key=lambda kv: kv[1][0] / kv[1][1])
        print(f"== {case}: worst against its bound {name} {v:.3e} (bound {tol:.1e})", flush=True)
    worst = max(((c, n, f["figure"], f["bound"]) for c, fs in per_case.items() for n, f in fs.items()),
                key=lambda t: t[2] / t[3])
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["device_errors"] = dict(
        what="the bound's figure of one training iteration on an MI355X with layers.LSTM, layers.ConvBNBlock and "
             "layers.Decoder swapped in: the larger of the figure against the float64 twin and the figure against the "
             "reference's float64 run, per case and tensor, with its bound",
        worst=dict(case=worst[0], tensor=worst[1], figure=worst[2], bound=worst[3]),
        all_within_bound=not failed, per_case=per_case)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"worst: {worst[0]} {worst[1]} {worst[2]:.3e} (bound {worst[3]:.1e}); wrote {args.out}")
    for f in failed:
        print("ABOVE THE BOUND:", f)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
