#!/usr/bin/env python3
"""Write tests/golden/resident_stop_late.npz: the resident batch-1 decoder's output digests for the
cases of tests/test_gpu_resident_stop_late.py (its collect()), to be run on the build of the
commit BEFORE the stop rule moved out of its own step into the next, never on the code under test:

    TTS_HIP_LIB=<that build's libtts_hip.so> python tools/make_resident_stop_late_golden.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import conftest  # noqa: E402  (puts the repository on sys.path)
import test_gpu_resident_stop_late as cases  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "resident_stop_late.npz"))
args = ap.parse_args()
res = cases.collect(conftest.golden_flags(conftest.golden("t2_fwdmask_L100")))
flat = {f"{case}_{k}": v for case, d in res.items() for k, v in d.items()}
np.savez_compressed(args.out, **flat)
print({case: int(d["frames"][0]) for case, d in res.items()}, os.path.getsize(args.out), "bytes")
