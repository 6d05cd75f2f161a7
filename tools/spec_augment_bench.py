"""Time of SpecAugment on the device (ctcn_spec_augment) by HIP events, at the recipe's base-feature shapes -- 32 x 800 x 81 and 8 x 800 x 81,
ragged by a few frames as a length-sorted batch is -- with masks only and with the time warp (the class defaults of
utils/features.SpecAugment), the augmentation and ops.frame_context back to back (0 / 2 / 2 / 2: the shipped splice), and, as the
yardsticks that this stage leaves unchanged, ops.frame_context alone and ops.fbank on 32 x 8 s of audio.

    python tools/spec_augment_bench.py [--reps 50] [--rounds 5] [--yardsticks-only]

Per round, alternating: `--reps` back-to-back calls of each variant after a warm-up of all; prints one JSON line with the median and the
spread of the per-call time over the rounds, the bytes the algorithm has to move (the base batch read once and written once) and the rate
that makes of the median.  --yardsticks-only, or a tree without ops.spec_augment, times the two yardsticks alone: the same command, copied
into a checkout of the parent commit, measures it like for like (what runs between two timed windows moves them by a few percent).  GPU
only: no device, no number.  """
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

MASKS = dict(num_freq_masks=2, freq_width=15, num_time_masks=2, time_width=40, time_ratio=0.2)
WARP = dict(MASKS, warp_window=5)
CONTEXT = dict(left=0, right=2, skip=2, n_downsample=2)


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
    ap.add_argument("--yardsticks-only", action="store_true", help="time ops.frame_context and ops.fbank alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spec_augment_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    have = hasattr(ops, "spec_augment") and not args.yardsticks_only
    T, F = 800, 81
    rs = np.random.RandomState(0)
    fns, algo = {}, {}
    for B in (32, 8):
        x = torch.from_numpy(rs.randn(B, T, F).astype(np.float32)).to(dev)
        frames = torch.tensor([T - 10 * (b % 7) for b in range(B)], dtype=torch.int32, device=dev)
        fns["frame_context_%dx%dx%d" % (B, T, F)] = lambda x=x, fr=frames: ops.frame_context(x, fr, **CONTEXT)
        algo["frame_context_%dx%dx%d" % (B, T, F)] = 4 * B * T * F + 4 * B * (T // 2) * 3 * F
        if not have:
            continue
        for name, kw in (("masks", MASKS), ("warp_masks", WARP)):
            key = "spec_augment_%s_%dx%dx%d" % (name, B, T, F)
            fns[key] = lambda x=x, fr=frames, kw=kw: ops.spec_augment(x, fr, 1, 0, **kw)
            algo[key] = 2 * 4 * B * T * F
        key = "spec_augment_warp_masks_then_frame_context_%dx%dx%d" % (B, T, F)
        fns[key] = lambda x=x, fr=frames: ops.frame_context(ops.spec_augment(x, fr, 1, 0, **WARP), fr, **CONTEXT)
        algo[key] = 2 * 4 * B * T * F + algo["frame_context_%dx%dx%d" % (B, T, F)]
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
    out = {"spec_augment": have, "reps": args.reps, "rounds": args.rounds, "us_per_call": {k: spread(v) for k, v in times.items()},
           "algorithmic_bytes": algo}
    out["algorithmic_GBps_at_median"] = {k: round(algo[k] / (out["us_per_call"][k]["median"] * 1e-6) / 1e9, 1) for k in algo}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
