#!/usr/bin/env python
"""Write profiles/postnet_contract.json: one record per checked call of
tests/test_gpu_postnet_contract.py (case, model, B, Tmax, frames, the kernel kind that served each
Postnet layer, the worst per-sentence relative RMS of the output and of the postnet term and the
worst max-abs against the fp64 oracle), each with the same figures of the fp32 oracle against the
fp64 oracle on the CPU, which is the floor a later, tighter bound for these stages has to stay
above; and the worst figures per kernel kind (a call counts for every kind among its layers).

    python tools/postnet_contract_report.py [--out profiles/postnet_contract.json] [pytest args]

Runs the contract tests in this process (on an MI355X) and collects what they recorded."""
import argparse
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

KIND_NAMES = ("small_channel_major", "small_tap32", "small_tap16", "tiled16", "splitk_reduce", "splitk_fused",
              "varlen64", "tiled32", "tiled64")
FIGURES = ("out_rel", "term_rel", "out_abs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "postnet_contract.json"))
    args, rest = ap.parse_known_args()
    import postnet_util as pu
    rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider",
                      os.path.join(REPO, "tests", "test_gpu_postnet_contract.py")] + rest)
    records = []
    for r in pu.RECORDS:
        sp = r["_specs"]
        mels = [pu.mel(T, k) for T, k in sp]
        f32 = pu.pad_out(r["model"], pu.ref_batch(r["model"], sp, np.float32))
        e = pu.postnet_errors(r["model"], f32, mels, pu.ref_batch(r["model"], sp))
        rec = {k: v for k, v in r.items() if not k.startswith("_")}
        rec["lens"] = [T for T, _ in sp]
        rec["fp32_oracle"] = {k: max(e[k]) for k in FIGURES if k in e}
        records.append(rec)
    worst = {}
    for r in records:
        groups = ["postcbhg"] if r["kinds"] is None else sorted({KIND_NAMES[k] for k in r["kinds"]})
        for g in groups + ["fp32_oracle_" + r["model"]]:
            src = r["fp32_oracle"] if g.startswith("fp32_oracle") else r
            w = worst.setdefault(g, {})
            for k in FIGURES:
                if k in src:
                    w[k] = max(w.get(k, 0.0), src[k])
    doc = dict(bounds=dict(MEL_RTOL=pu.MEL_RTOL, ALIGN_ATOL=pu.ALIGN_ATOL), kind_names=list(KIND_NAMES),
               pytest_exit=int(rc), worst=worst, records=records)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {len(records)} records to {args.out} (pytest exit {int(rc)}); worst: {json.dumps(worst)}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
