#!/usr/bin/env python
"""Write profiles/tacotron_encoder_contract.json: one record per checked case of
tests/test_gpu_tacotron_encoder_contract.py (case, model, B, Lmax, frames, the ConvKind of the
eleven launches of each call, the worst per-sentence relative RMS and max-abs of the encoder,
speaker and style terms against the fp64 oracle), each with the fp32 oracle's figures on the same
inputs beside it (the fp32 oracle performing the same subtraction for the speaker and style
terms); the worst figures per term and model; the bounds; the sharpening recipe; and the
smallest movement of its term by each oracle mutant over the shapes of the cases.

    python tools/tacotron_encoder_contract_report.py [--out profiles/tacotron_encoder_contract.json] [pytest args]

Runs the contract tests in this process (on an MI355X) and collects what they recorded."""
import argparse
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

KIND_NAMES = ("small_channel_major", "small_tap32", "small_tap16", "tiled16", "splitk_reduce", "splitk_fused",
              "varlen64", "tiled32", "tiled64")


def _max(pairs):
    pairs = list(pairs)
    return dict(rel=max(r for r, _ in pairs), abs=max(a for _, a in pairs))


def fp32_figures(u, r):
    """The fp32 oracle's worst figures on the sentences record ``r`` compared with the fp64 oracle."""
    sp = r["_sp"]
    sel = range(len(sp)) if r["_check"] is None else r["_check"]
    f = dict(encoder=_max(u.f32_encoder(r["model"], *sp[b]) for b in sel))
    if "speaker" in r:
        f["speaker"] = _max(u.f32_speaker(*sp[b], r["_speakers"][b]) for b in range(len(sp)))
    if "style" in r:
        f["style"] = _max(u.f32_style(r["model"], *sp[b], *r["_styles"][b]) for b in sel)
    return f


def mutant_margins(u):
    """Smallest relative-RMS movement of its term by each mutant over the shapes of the GPU cases
    (where it is not the identity), and the margin the CPU test holds it to."""
    import test_tacotron_encoder_util_cpu as c
    least = {}
    for L, k, Lmax in c._cbhg_shapes():
        for m in u.CBHG_MUTANTS:
            if not u.mutant_is_identity(m, L=L, Lmax=Lmax):
                rel = u.vec_errors(u.encoder_mutant(u.GSTM, L, k, m, Lmax), u.enc_ref(u.GSTM, L, k))[0]
                least[m] = min(least.get(m, rel), rel)
    o = u.oracle(u.SHARP)
    for Ts, k, nxt in c._style_shapes():
        for m in u.GST_MUTANTS:
            if not u.mutant_is_identity(m, Ts=Ts, B=1 if nxt is None else 5):
                got = u.gst_mutant(o, u.style_of(Ts, k), m, None if nxt is None else u.style_of(Ts, nxt))
                rel = u.vec_errors(got, u.gst_ref(u.SHARP, Ts, k))[0]
                least[m] = min(least.get(m, rel), rel)
    need = {m: u.MARGIN * (u.MEL_RTOL if m in u.CBHG_MUTANTS else u.STYLE_REL[u.SHARP]) for m in least}
    return {m: dict(least_rel=least[m], required_rel=need[m]) for m in least}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tacotron_encoder_contract.json"))
    args, rest = ap.parse_known_args()
    import tacotron_encoder_util as u
    rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider",
                      os.path.join(REPO, "tests", "test_gpu_tacotron_encoder_contract.py")] + rest)
    records, worst, kinds_seen = [], {}, {}
    for r in u.RECORDS:
        rec = {k: v for k, v in r.items() if not k.startswith("_")}
        rec["lens"] = [L for L, _ in r["_sp"]]
        if r["_styles"] is not None:
            rec["style_frames"] = r["_styles"][0][0]
        rec["fp32_oracle"] = fp32_figures(u, r)
        records.append(rec)
        for term in ("encoder", "speaker", "style"):
            if term in rec:
                for src, name in ((rec, "kernel"), (rec["fp32_oracle"], "fp32_oracle")):
                    w = worst.setdefault(f"{term}_{r['model']}", {}).setdefault(name, dict(rel=0.0, abs=0.0))
                    w["rel"], w["abs"] = max(w["rel"], src[term]["rel"]), max(w["abs"], src[term]["abs"])
        for call, kk in rec["kinds"].items():
            key = "frames<=4096" if rec["frames"] <= 4096 else "frames>4096"
            names = [KIND_NAMES[k] if k >= 0 else "none" for k in kk]
            kinds_seen.setdefault(key, {}).setdefault(",".join(names), 0)
            kinds_seen[key][",".join(names)] += 1
    bounds = dict(MEL_RTOL=u.MEL_RTOL, ALIGN_ATOL=u.ALIGN_ATOL, ENC_REL=u.ENC_REL, ENC_ABS=u.ENC_ABS, SPK_REL=u.SPK_REL,
                  SPK_ABS=u.SPK_ABS, STYLE_REL=u.STYLE_REL, STYLE_ABS=u.STYLE_ABS)
    doc = dict(bounds=bounds, sharpen=[list(x) for x in u.SHARPEN], kind_names=list(KIND_NAMES), pytest_exit=int(rc),
               worst=worst, kinds_seen=kinds_seen, mutants=mutant_margins(u), records=records)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {len(records)} records to {args.out} (pytest exit {int(rc)}); worst: {json.dumps(worst)}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
