#!/usr/bin/env python3
"""Writes tests/golden/ctc_parent_bits.npz, the fixture of tests/test_ctc_parent_bits.py: the cases of that test, run on a build of the PARENT
of the commit that changes the CTC kernels -- check the parent out (or point CTCN_LIBCTCN at a library built from it), build, run

    tools/record_ctc_bits.py --commit <the parent's hash> [--out FILE]

on the GPU, and commit the file with the change.  Never run it on the code under test: the fixture would then prove nothing."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import test_ctc_parent_bits as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
ap.add_argument("--out", default=T.FIXTURE)
args = ap.parse_args()

from ctc_pytorch_amd import _lib  # noqa: E402

for name in sorted(T.CASES):                  # before anything is recorded: the infeasible, bad-length, tie ... cases are what they claim to be
    T.check_claims(name)
dev = torch.device("cuda:0")
arrays, meta = {}, {"commit": args.commit, "library": os.path.basename(_lib.SO_PATH), "cases": {}, "inputs": {}, "digests": {}}
for name in sorted(T.CASES):
    got, again = T.run_case(name, dev), T.run_case(name, dev)
    assert sorted(got) == sorted(again) and all(np.array_equal(got[k], again[k]) for k in got), "%s: two runs of the parent differ" % name
    meta["cases"][name] = sorted(got)
    meta["inputs"][name] = T.inputs_digest(name)
    for key, a in got.items():
        if a.size <= T.FULL_MAX:
            arrays["%s/%s" % (name, key)] = a
        else:
            meta["digests"]["%s/%s" % (name, key)] = T.digest(a)
    print("%-24s %3d outputs, %d of them as digests" % (name, len(got), sum(a.size > T.FULL_MAX for a in got.values())), flush=True)
arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
np.savez_compressed(args.out, **arrays)
print("wrote %s: %d bytes" % (args.out, os.path.getsize(args.out)))
