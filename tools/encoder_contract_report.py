#!/usr/bin/env python
"""Write profiles/encoder_contract.json: one record per checked call of
tests/test_gpu_encoder_contract.py (case, handle, B, Lmax, serving path, the worst per-sentence
relative RMS and max-abs of out / h_n / c_n against the fp64 oracle), each with the same figures of
the fp32 oracle against the fp64 oracle on the CPU, which is the floor a later, tighter bound for
this stage has to stay above.

    python tools/encoder_contract_report.py [--out profiles/encoder_contract.json] [pytest args]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "encoder_contract.json"))
    args, rest = ap.parse_known_args()
    import encoder_util as eu
    rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider",
                      os.path.join(REPO, "tests", "test_gpu_encoder_contract.py")] + rest)
    o32 = eu.oracle(np.float32)
    records = []
    for r in eu.RECORDS:
        ids, state = r["_ids"], r["_state"]
        states = None if state is None else eu.split_state(state)
        ref, ref_st = eu.ref_encoder_batch(eu.oracle(), ids, states)
        f32, f32_st = eu.ref_encoder_batch(o32, ids, states)
        e = eu.encoder_errors(f32, ref, [len(x) for x in ids], f32_st, ref_st)
        rec = {k: v for k, v in r.items() if not k.startswith("_")}
        rec["fp32_oracle"] = {k: max(v) for k, v in e.items() if k not in ("c_ref_max", "pad_nonzero")}
        records.append(rec)
    worst = {}
    for r in records:
        w = worst.setdefault(f"path{r['path']}", {})
        for k in ("out_rel", "out_abs", "h_rel", "h_abs", "c_rel", "c_abs"):
            if k in r:
                w[k] = max(w.get(k, 0.0), r[k])
        f = worst.setdefault("fp32_oracle", {})
        for k, v in r["fp32_oracle"].items():
            f[k] = max(f.get(k, 0.0), v)
    doc = dict(bounds=dict(MEL_RTOL=eu.MEL_RTOL, ALIGN_ATOL=eu.ALIGN_ATOL), pytest_exit=int(rc), worst=worst,
               records=records)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {len(records)} records to {args.out} (pytest exit {int(rc)}); worst: {json.dumps(worst)}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
