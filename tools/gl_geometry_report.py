#!/usr/bin/env python
"""Write profiles/gl_geometry.json: per STFT geometry of tests/gl_geometry_util.py and per run of
tests/test_gpu_gl_geometry.py, the worst per-sentence relative RMS of the Griffin-Lim waveform against
the oracle and the iteration loop the run took, and per geometry the analysis half's worst errors.

    python tools/gl_geometry_report.py [--out profiles/gl_geometry.json] [pytest args]

Runs the geometry tests in this process (on an MI355X) and collects what they measured."""
import argparse
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gl_geometry.json"))
    args, rest = ap.parse_known_args()
    rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider",
                      os.path.join(REPO, "tests", "test_gpu_gl_geometry.py")] + rest)
    import gl_geometry_util as G
    t = sys.modules["test_gpu_gl_geometry"]
    geo = {}
    for name in G.NAMES:
        hop, win = G.hop_win(name)
        woff, fb, winp = G._geo(hop, win)
        geo[name] = dict(hop=hop, win=win, woff=woff, fb=fb, winp=winp, contributors=(win + hop - 1) // hop,
                         first_F_gather_misfit=next((F for F in range(2, 45) if not G.gather_fits(hop, win, F)), None),
                         griffin_lim=[], analysis=None)
    for key, r in t._GPU.items():
        if key[0] == "analysis":
            geo[key[1]]["analysis"] = dict(N=r["N"], F=r["F"], linear_max_err=max(r["lin_err"]),
                                           mel_max_err=max(r["mel_err"]), tol=min(r["lin_tol"] + r["mel_tol"]),
                                           features_bitwise=r["bitwise"])
            continue
        name, run, iters, mode, _ = key
        worst = max(range(len(r["rel"])), key=lambda i: r["rel"][i])
        geo[name]["griffin_lim"].append(dict(run=run, env=t.RUNS[run][1], iters=iters, mode="linear" if mode else "mel",
                                             frames=r["Fs"], path=r["path"], worst_rel_rms=r["rel"][worst],
                                             worst_F=r["Fs"][worst], padding_zero=r["pad_zero"]))
    worst = {}
    for name, g in geo.items():
        for r in g["griffin_lim"]:
            k = "zero_iterations" if r["iters"] == 0 else "with_iterations"
            if r["worst_rel_rms"] > worst.get(k, (0.0,))[0]:
                worst[k] = (r["worst_rel_rms"], name, r["run"], r["iters"], r["worst_F"])
    doc = dict(what="Griffin-Lim and analysis kernels at twelve STFT geometries on one MI355X against the CPU oracle "
                    "(tests/test_gpu_gl_geometry.py): worst per-sentence relative RMS per run, and the loop taken",
               bounds=dict(ZERO_RTOL=t.ZERO_RTOL, WAV_RTOL=t.WAV_RTOL, analysis="1e-5 * max(1, |ref|max)"),
               pytest_exit=int(rc), worst=worst, geometries=geo)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out} (pytest exit {int(rc)}); worst: {json.dumps(worst)}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
