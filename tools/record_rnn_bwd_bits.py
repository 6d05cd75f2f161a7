#!/usr/bin/env python3
"""Writes tests/golden/rnn_bwd_parent_bits.npz, the fixture of tests/test_rnn_bwd_chain.py: the cases of that test, run on a build of the PARENT
of the commit that changes the backward recurrences -- check the parent out (or point CTCN_LIBCTCN at a library built from it), build, run

    tools/record_rnn_bwd_bits.py --commit <the parent's hash> [--out FILE]

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
import test_rnn_bwd_chain as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
ap.add_argument("--out", default=T.FIXTURE)
args = ap.parse_args()

from ctc_pytorch_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
wrong = []
arrays, meta = {}, {"commit": args.commit, "library": os.path.basename(_lib.SO_PATH), "kernels": {}, "digests": {}}
for name in sorted(T.CASES):
    got, kernels = T.run_case(name, dev)
    again, kernels2 = T.run_case(name, dev)
    assert kernels == kernels2 and all(np.array_equal(got[k], again[k]) for k in got), "%s: two runs of the parent differ" % name
    if kernels[1] != T.CASES[name][9]:
        wrong.append("%s ran %s, the case is about %s" % (name, kernels, T.CASES[name][9]))
    meta["kernels"][name] = list(kernels)
    for key, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), (name, key)
        if a.size <= T.FULL_MAX:
            arrays["%s/%s" % (name, key)] = a
        else:
            meta["digests"]["%s/%s.sha256" % (name, key)] = T.digest(a)
            arrays["%s/%s.sample" % (name, key)] = np.ascontiguousarray(T.sample_of(a))
    print("%-22s %-18s %-18s %s" % (name, kernels[0], kernels[1], " ".join("%s%s" % (k, list(v.shape)) for k, v in got.items())), flush=True)
assert not wrong, "nothing written -- " + "; ".join(wrong)
arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
np.savez(args.out, **arrays)
print("wrote %s: %d bytes" % (args.out, os.path.getsize(args.out)))
