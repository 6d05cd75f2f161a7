#!/usr/bin/env python3
"""Writes the fixture of a "same bits as the parent" test (tests/test_ctc_parent_bits.py -> tests/golden/ctc_parent_bits.npz,
tests/test_frontend_parent_bits.py -> tests/golden/frontend_parent_bits.npz): the cases of that test, run on a build of the PARENT of the
commit that changes the kernels -- check the parent out (or point CTCN_LIBCTCN at a library built from it), build, run

    tools/record_parent_bits.py --test <module under tests/> --commit <the parent's hash> [--out FILE]

on the GPU, and commit the file with the change.  Never run it on the code under test: the fixture would then prove nothing.  The test
module supplies CASES, check_claims, run_case, inputs_digest, digest, FULL_MAX and FIXTURE."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--test", required=True, help="the test module whose cases are recorded, e.g. test_frontend_parent_bits")
ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
ap.add_argument("--out", default=None, help="default: the test's FIXTURE")
args = ap.parse_args()
T = importlib.import_module(args.test[:-3] if args.test.endswith(".py") else args.test)
out_path = args.out or T.FIXTURE

from ctc_pytorch_amd import _lib  # noqa: E402

for name in sorted(T.CASES):                  # before anything is recorded: the cases are what they claim to be
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
np.savez_compressed(out_path, **arrays)
print("wrote %s: %d bytes" % (out_path, os.path.getsize(out_path)))
