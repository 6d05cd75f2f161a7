"""Time of the device context stage (ctcn_frame_context: deltas, splice, skip, downsample pad) and what it takes off the host.

    python tools/frame_context_bench.py [--reps 200] [--rounds 5] [--frames 800] [--feat-dim 81] [--batches 20]

1. Call time by HIP events, alternating rounds of `--reps` back-to-back calls of each variant after a warm-up of all: ops.frame_context on
   32 x 800 x 81 and 8 x 800 x 81 (the shipped batch size) under the shipped context (left 0, right 2, skip 2, n_downsample 2: 243
   columns), and on 32 x 800 x 13 with two delta orders (13 -> 39, no splice).  Beside each the bytes the call has to move -- the real base
   frames once, the padded output once -- and the rate that makes of the median.  The call includes what ops.frame_context does around the
   launch (three allocations, the upload of B frame counts when they come as a list; here they are a device tensor).
2. Host cost per batch of the two loader paths over the same synthetic archive (`--batches` batches of 8 utterances of `--frames` x
   `--feat-dim`, ragged by a few frames): SpeechDataset.__getitem__ x 8, the collate, the copy into pinned staging memory -- wall clock,
   medians over the batches -- and the bytes each path sends over PCIe.  Host path: the spliced batch; device path: the base batch, plus
   the host time to enqueue the one launch.

Prints one JSON line.  GPU only: no device, no number.  """
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_pytorch_amd import ops                                    # noqa: E402
from ctc_pytorch_amd.utils import data_loader as DL                # noqa: E402
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


class _Opts(object):
    left_ctx, right_ctx, n_skip_frame, n_downsample = 0, 2, 2, 2


def host_cost(dev, frames, feat_dim, batches, batch_size=8):
    """Per-batch host time of the two loader paths, segment by segment, and their H2D bytes."""
    rs = np.random.RandomState(1)
    ctx = features.FrameContext.from_opts(_Opts)
    with tempfile.TemporaryDirectory() as tmp:
        n = batches * batch_size
        mats = {"utt%04d" % i: rs.standard_normal((frames - (i % 7), feat_dim)).astype(np.float32) for i in range(n)}
        ark, scp, lab, units = (os.path.join(tmp, f) for f in ("feats.ark", "feats.scp", "text", "units"))
        DL.write_kaldi_ark(ark, scp, mats)
        with open(units, "w") as f:
            f.write("a\nb\nc\n")
        with open(lab, "w") as f:
            for utt in mats:
                f.write("%s %s\n" % (utt, " ".join("abc"[k % 3] for k in range(40))))
        vocab = DL.Vocab(units)
        out = {}
        for name, base in (("host_path", False), ("device_context_path", True)):
            ds = DL.SpeechDataset(vocab, scp, lab, _Opts, base_features=base)
            collate = DL.create_base_input if base else DL.create_input
            slot = {"bufs": {}, "copied": None}
            seg = {"getitem_us": [], "collate_us": [], "pinned_copy_us": [], "enqueue_us": []}
            h2d = 0
            for rep in range(2):                                       # the first pass warms the page cache and sizes the pinned buffers
                for k in range(batches):
                    t0 = time.perf_counter()
                    items = [ds[i] for i in range(k * batch_size, (k + 1) * batch_size)]
                    t1 = time.perf_counter()
                    batch = collate(items)
                    t2 = time.perf_counter()
                    pinned = [DL.DevicePrefetcher._pinned(slot, j, t) for j, t in enumerate(batch[:4])]
                    t3 = time.perf_counter()
                    staged = [t.to(dev, non_blocking=True) for t in pinned]
                    t4 = time.perf_counter()
                    if base:
                        ctx(staged[0], staged[1])
                    t5 = time.perf_counter()
                    torch.cuda.synchronize()
                    if rep:
                        for key, v in zip(seg, (t1 - t0, t2 - t1, t3 - t2, t5 - t4)):
                            seg[key].append(v * 1e6)
                        h2d += sum(t.numel() * t.element_size() for t in pinned)
            res = {key: spread(v) for key, v in seg.items() if base or key != "enqueue_us"}
            res["host_total_us_median"] = round(sum(r["median"] for r in res.values()), 1)
            res["h2d_bytes_per_batch"] = h2d // batches
            out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--feat-dim", type=int, default=81)
    ap.add_argument("--batches", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frame_context_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    T, F = args.frames, args.feat_dim
    fns, algo, shapes = {}, {}, {}
    for key, B, dim, kw in (("splice_B32", 32, F, dict(left=0, right=2, skip=2, n_downsample=2)),
                            ("splice_B8", 8, F, dict(left=0, right=2, skip=2, n_downsample=2)),
                            ("deltas2_B32_13", 32, 13, dict(delta_order=2, delta_window=2))):
        x = torch.randn((B, T, dim), device=dev)
        lens = [T - (b % 7) for b in range(B)]
        fr = torch.tensor(lens, dtype=torch.int32, device=dev)
        fns[key] = lambda x=x, fr=fr, kw=kw: ops.frame_context(x, fr, **kw)
        out, _, _ = fns[key]()
        shapes[key] = {"in": [B, T, dim], "out": list(out.shape), "tile_rows": ops.frame_context_tile(dim, **kw)}
        algo[key] = 4 * sum(lens) * dim + 4 * out.numel()              # the real base frames once, the padded output once
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    res = {"reps": args.reps, "rounds": args.rounds, "shapes": shapes, "us_per_call": {k: spread(v) for k, v in times.items()},
           "algorithmic_bytes": algo}
    res["algorithmic_GBps_at_median"] = {k: round(algo[k] / (res["us_per_call"][k]["median"] * 1e-6) / 1e9, 1) for k in algo}
    res["host_cost_per_batch_of_8"] = host_cost(dev, T, F, args.batches)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
