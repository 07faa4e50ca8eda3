"""Oracle parity of the resident TacotronGST decoder at its slice, group and queue edges, as a report: every
case of tests/tacotron_resident_util.py on the device, each sentence the case table sends through the float64
oracle compared by check_sentence; per case the worst alignment, stop and mel figure, the share of steps left
out of the argmax comparison, the step counts and the path that served it, and whether the first B sentences of
the group-shape batch carry the bits they have in the B = 32 run.  Prints a line per case and writes all of it
into profiles/tacotron_resident_contract.json.  Needs an MI355X:

    python tools/tacotron_resident_report.py [--out profiles/tacotron_resident_contract.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import tacotron_resident_util as u  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tacotron_resident_contract.json"))
    args = ap.parse_args()
    models, per_case, failed = {}, {}, []

    def model(c):
        key = (c["r"], c["m"], tuple(sorted(c["model_kw"].items())))
        if key not in models:
            models[key] = u.make_model(c["r"], c["m"], c["cap"], **c["model_kw"])
        return models[key]

    def compare(name, res, pairs):
        figs = []
        for b, i in pairs:
            try:
                figs.append(u.check_sentence(u.sentence(res, b), u.case_reference(name, i), u.CASES[name]["sents"][i].L))
            except AssertionError as e:
                failed.append(f"{name} sentence {i}: {e}")
        return figs

    for name, c in u.CASES.items():
        res = u.run_case(model(c), name)
        figs = compare(name, res, [(i, i) for i in c["oracle"]])
        if name == "slice_edges" or name.startswith("mel_"):  # the sentences that also run alone
            for i in (c["oracle"] if name == "slice_edges" else (0,)):
                figs += compare(name, u.run(model(c), c["sents"][i:i + 1], c["cap"]), [(0, i)])
        if res["resident"] is not c["resident"]:
            failed.append(f"{name}: served by the other path")
        rec = dict(u.worst(figs)) if figs else {}
        rec.update(lens=res["lens"], steps=res["steps"], cap=c["cap"], r=c["r"], memory_size=c["m"],
                   resident=res["resident"], sentences_vs_oracle=list(c["oracle"]))
        if name == "groups":
            same = {}
            for B in u.GROUP_BS[:-1]:
                part = u.run_case(model(c), name, first=B)
                same[str(B)] = all(u.same_bits(u.sentence(part, b), u.sentence(res, b), u.GROUP_LENS[b])
                                   for b in range(B))
            rec["batch_invariance_bitwise"] = same
            rec["batch_invariance_note"] = ("B = 1 differs ahead of the kernel: the go frame's prenet layer-1 GEMM "
                                            "serves B = 1 with VALU dot products, B >= 2 with MFMA tiles")
        per_case[name] = rec
        print(f"== {name}: resident {res['resident']}, steps {min(res['steps'])}..{max(res['steps'])}, " +
              ", ".join(f"{k} {v:.3g}" for k, v in rec.items() if isinstance(v, float)), flush=True)
    keys = ("align_err", "stop_err", "mel_rel_rms", "skipped_argmax_share")
    doc = dict(
        what="resident TacotronGST decoder (and the multi-launch path where it ends) on an MI355X against the "
             "float64 numpy oracle's decoder on the same float32 encoder rows: per case the worst max-abs alignment "
             "and stop error, mel relative RMS and share of steps left out of the argmax comparison over the "
             "sentences compared, with every sentence's step count",
        bounds=dict(align_err=u.ATOL, stop_err=u.ATOL, mel_rel_rms=u.RTOL, skipped_argmax_share=u.SKIP_CAP),
        worst={k: max((c[k], n) for n, c in per_case.items() if k in c) for k in keys},
        all_within_bound=not failed, per_case=per_case)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print("worst: " + ", ".join(f"{k} {v[0]:.3g} ({v[1]})" for k, v in doc["worst"].items()) + f"; wrote {args.out}")
    for f in failed:
        print("ABOVE THE BOUND:", f)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
