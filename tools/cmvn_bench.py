"""Time of the grouped and the sliding-window CMVN on the device by HIP events, at the recipe's base-feature shapes -- 32 x 800 x 81 and
8 x 800 x 81, ragged by a few frames as a length-sorted batch is:
  cmvn_accumulate_groups at G = 1 and G = 32 beside ctcn_cmvn_accumulate on the same batch (the partial kernel is shared; the global call
  is the grouped finish without ids, so it reads what G = 1 reads -- on a parent of that change the difference is the global finish kernel's);
  cmvn_apply (out of place, into a preallocated tensor) against the bytes it has to move, and the same call on a 1 x 1 x 81 batch: the
  time of a launch that has nothing to do, i.e. the part of the call that is overhead and not the kernel;
  cmvn_sliding at Kaldi's defaults with and without the variance, also as ns per frame of the utterance (the chain in time);
and, as the yardsticks this stage leaves unchanged, ops.cmvn_accumulate and ops.fbank on 32 x 8 s of audio.

    python tools/cmvn_bench.py [--reps 50] [--rounds 5] [--yardsticks-only]

Per round, alternating: `--reps` back-to-back calls of each variant after a warm-up of all; prints one JSON line with the median and the
spread of the per-call time over the rounds.  --yardsticks-only, or a tree without ops.cmvn_apply, times the two yardsticks alone: the same
command, copied into a checkout of the parent commit, measures it like for like.  GPU only: no device, no number.  """
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_pytorch_amd import ops                                    # noqa: E402
from ctc_pytorch_amd.utils import features                         # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                          # us per call


def spread(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--yardsticks-only", action="store_true", help="time ops.cmvn_accumulate and ops.fbank alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cmvn_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    have = hasattr(ops, "cmvn_apply") and not args.yardsticks_only
    T, F = 800, 81
    rs = np.random.RandomState(0)
    fns, algo = {}, {}
    for B in (32, 8):
        shape = "%dx%dx%d" % (B, T, F)
        x = torch.from_numpy((2.0 * rs.randn(B, T, F) + 5.0).astype(np.float32)).to(dev)
        frames = torch.tensor([T - 10 * (b % 7) for b in range(B)], dtype=torch.int32, device=dev)
        stats = torch.zeros(2, F + 1, dtype=torch.float64, device=dev)
        fns["cmvn_accumulate_" + shape] = lambda x=x, fr=frames, s=stats: ops.cmvn_accumulate(x, fr, s)
        algo["cmvn_accumulate_" + shape] = 4 * B * T * F
        if not have:
            continue
        for G in (1, 32):
            ids = torch.tensor([b % G for b in range(B)], dtype=torch.int32, device=dev)
            gs = torch.zeros(G, 2, F + 1, dtype=torch.float64, device=dev)
            fns["cmvn_accumulate_groups_G%d_%s" % (G, shape)] = lambda x=x, fr=frames, i=ids, s=gs: ops.cmvn_accumulate_groups(x, fr, i, s)
            algo["cmvn_accumulate_groups_G%d_%s" % (G, shape)] = 4 * B * T * F
        ids = torch.tensor([b % 8 for b in range(B)], dtype=torch.int32, device=dev)
        gs = ops.cmvn_accumulate_groups(x, frames, ids, torch.zeros(8, 2, F + 1, dtype=torch.float64, device=dev))
        out = torch.empty_like(x)
        fns["cmvn_apply_" + shape] = lambda x=x, fr=frames, i=ids, s=gs, o=out: ops.cmvn_apply(x, fr, s, i, out=o)
        algo["cmvn_apply_" + shape] = 2 * 4 * B * T * F
        for nv in (False, True):
            key = "cmvn_sliding_%s_%s" % ("var" if nv else "mean", shape)
            fns[key] = lambda x=x, fr=frames, o=out, nv=nv: ops.cmvn_sliding(x, fr, normalize_variance=nv, out=o)
            algo[key] = 2 * 4 * B * T * F
    if have:
        x1, f1 = torch.zeros(1, 1, F, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
        s1, o1 = torch.ones(1, 2, F + 1, dtype=torch.float64, device=dev), torch.empty(1, 1, F, device=dev)
        fns["cmvn_apply_1x1x81"] = lambda: ops.cmvn_apply(x1, f1, s1, out=o1)
    fb = features.Fbank(features.FbankConfig(window_type="hamming", num_mel_bins=80, use_energy=True, dither=0.0), dev)
    N = 8 * 16000
    w16 = torch.from_numpy(np.clip(np.round(3000.0 * rs.standard_normal((32, N))), -32768, 32767).astype(np.int16)).to(dev)
    lens = [N - 160 * (b % 7) for b in range(32)]
    fns["fbank_int16_32x8s"] = lambda: ops.fbank(w16, lens, fb.plan)
    algo["fbank_int16_32x8s"] = 2 * 32 * N + 4 * fb.feat_dim * fb.num_frames(N) * 32
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    out = {"cmvn": have, "reps": args.reps, "rounds": args.rounds, "us_per_call": {k: spread(v) for k, v in times.items()},
           "algorithmic_bytes": algo}
    out["algorithmic_GBps_at_median"] = {k: round(algo[k] / (out["us_per_call"][k]["median"] * 1e-6) / 1e9, 1) for k in algo}
    out["sliding_ns_per_frame_at_median"] = {k: round(v["median"] * 1e3 / T, 1) for k, v in out["us_per_call"].items() if k.startswith("cmvn_sliding")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
