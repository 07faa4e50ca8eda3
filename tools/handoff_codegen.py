#!/usr/bin/env python3
"""Generated-code comparison of the persistent kernels between two source trees (CPU only).

  tools/handoff_codegen.py <parent csrc dir> <new csrc dir> [> profiles/handoff_refactor_codegen.txt]

Compiles the five translation units that hold a persistent kernel in both trees with the Makefile's
flags plus --cuda-device-only -S and compares, per persistent kernel instantiation, the resources
(VGPRs, AGPRs, next_free_sgpr, scratch, LDS, occupancy) and the counts of the hand-off protocol's
instructions (s_sleep, clock reads, sc1 accesses, s_getreg_b32).  A recorder: every figure that
differs is marked, for the record to explain; the code length is reported only.  Exit status 1 if
a marked figure differs."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

UNITS = ["resident_decoder", "resident_batch", "tacotron_resident", "encoder_resident", "griffin_lim"]
PERSISTENT = re.compile(r"resident_(decoder_|batch_)?kernel|gl_persistent")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-ffp-contract=off", "--cuda-device-only", "-S"]
GATED = ["vgpr", "agpr", "sgpr", "scratch", "lds", "occ", "s_sleep", "clock", "sc1", "s_getreg"]


def compile_unit(src_dir, unit, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + FLAGS + [unit + ".hip", "-o", out], cwd=src_dir, stderr=subprocess.PIPE, text=True)
    # (the driver's own note that --hip-link is unused with -S is not the unit's)
    msg = "\n".join(l for l in r.stderr.splitlines() if "--hip-link" not in l)
    if msg.strip():
        sys.stderr.write("%s/%s.hip:\n%s\n" % (src_dir, unit, msg))
    if r.returncode:
        raise SystemExit("%s/%s.hip did not compile" % (src_dir, unit))


def kernels(path):
    """{demangled-ish name: figures} of every persistent kernel in one .s file"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel(.*?); Occupancy: (\d+)",
                         text, re.S | re.M):
        name, body, desc, info, occ = m.groups()
        if not PERSISTENT.search(name):
            continue
        ins = [l.split(";")[0].strip() for l in body.splitlines()]
        ins = [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]
        grab = lambda pat, s: int(re.search(pat, s).group(1))
        out[name] = {
            "vgpr": grab(r"; NumVgprs: (\d+)", info),
            "agpr": grab(r"; NumAgprs: (\d+)", info),
            "sgpr": grab(r"\.amdhsa_next_free_sgpr (\d+)", desc),
            "scratch": grab(r"; ScratchSize: (\d+)", info),
            "lds": grab(r"; LDSByteSize: (\d+)", info),
            "occ": int(occ),
            "s_sleep": sum(l.startswith("s_sleep") for l in ins),
            "clock": sum(l.startswith(("s_memrealtime", "s_sendmsg_rtn")) for l in ins),
            "sc1": sum(bool(re.search(r"\bsc1\b", l)) for l in ins),
            "s_getreg": sum(l.startswith("s_getreg_b32") for l in ins),
            "bytes": grab(r"; codeLenInByte = (\d+)", info),
        }
    return out


def short(name):
    """kernel name with its template arguments decoded (bools and ints)"""
    m = re.search(r"\d+((?:tacotron_|encoder_)?resident\w*?kernel|gl_persistent\w*?kernel)(?:I((?:L[bi]\d+E)+)E)?", name)
    if not m:
        return name
    args = re.findall(r"L[bi](\d+)E", m.group(2) or "")
    return m.group(1) + ("<" + ", ".join(args) + ">" if args else "")


def main():
    parent, new = sys.argv[1], sys.argv[2]
    bad = 0
    print("# Persistent kernels, parent vs new: hipcc %s" % " ".join(FLAGS))
    print("# compared: %s; reported: bytes (codeLenInByte)" % ", ".join(GATED))
    print("# template arguments: resident_decoder <PROF, GEN>, resident_batch <NB, PROF, GEN>, tacotron_resident <QUEUE>")
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(d, u, os.path.join(tmp, "%s_%s.s" % (u, tag))) for u in UNITS for tag, d in (("parent", parent), ("new", new))]
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(lambda j: compile_unit(*j), jobs))
        for u in UNITS:
            fig = [kernels(os.path.join(tmp, "%s_%s.s" % (u, tag))) for tag in ("parent", "new")]
            if set(fig[0]) != set(fig[1]):
                print("%s: kernel sets differ: %s" % (u, sorted(set(fig[0]) ^ set(fig[1]))))
                bad += 1
            for k in sorted(set(fig[0]) & set(fig[1])):
                a, b = fig[0][k], fig[1][k]
                diff = [g for g in GATED if a[g] != b[g]]
                bad += len(diff)
                print("%s %s" % (u, short(k)))
                print("    " + " ".join("%s=%s" % (g, a[g] if a[g] == b[g] else "%d->%d" % (a[g], b[g])) for g in GATED))
                print("    bytes %d -> %d (%+.2f %%)   %s" % (a["bytes"], b["bytes"], 100.0 * (b["bytes"] - a["bytes"]) / a["bytes"],
                                                              "DIFFERS: " + ",".join(diff) if diff else "equal"))
    print("# %s" % ("all compared figures equal" if not bad else "%d compared figures differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
