"""What gradient-norm clipping and the non-finite-step guard cost per training step, and the norm kernel against its HBM floor.

    python tools/clip_bench.py [--workloads cfg2,cfg4] [--rounds 5] [--steps 20] [--prewarm 40]

Per workload, in ONE process, through the step closure bench.py times (bench.make_training_step: forward -> CTC / B -> backward ->
all-reduce -> FlatAdam.step, paced two steps ahead like run_epoch): three arrangements of the SAME optimiser object
    off    max_grad_norm=None, skip_nonfinite=False      (the plain fused Adam: the arrangement of every number published so far)
    clip   max_grad_norm=1.0                             (norm -> control -> Adam reading the coefficient)
    guard  max_grad_norm=1.0, skip_nonfinite=True
timed in `--rounds` alternating rounds of `--steps` steps each (host clock around a block that ends in a device synchronise) after
`--prewarm` untimed steps; prints median, min and max of the per-step time of each arrangement and the differences of the medians.
Then ctcn_grad_norm alone on the workload's flat gradient (HIP events around back-to-back calls: the chunk kernel + the one-workgroup
finalisation) against 4n bytes at the HBM peak bench.py's rooflines use (8.0 TB/s) and at the measured float4-copy rate (6.29 TB/s).
One JSON line per workload.  """
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                       # noqa: E402
from ctc_pytorch_amd import ops                                    # noqa: E402

ARRANGEMENTS = (("off", None, False), ("clip", 1.0, False), ("guard", 1.0, True))
HBM_COPY_GBS = 6290.0                                              # measured float4 copy on the MI355X


def block_ms(paced, steps, first):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        paced(first + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def events_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2,cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--prewarm", type=int, default=bench.PREWARM)
    ap.add_argument("--norm-reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    for name in args.workloads.split(","):
        c = bench.WORKLOADS[name]
        ts = bench.make_training_step(c, dev, 0, 1)
        opt, paced = ts["opt"], ts["paced"]

        def arrange(max_norm, guard):
            opt.step_count                      # after guarded steps this fetches the device counter: here, not inside a timed block
            opt.max_grad_norm, opt.skip_nonfinite = max_norm, guard

        k = 0
        for _, mx, gd in ARRANGEMENTS:                              # every arrangement's kernels are loaded before anything is timed
            arrange(mx, gd)
            for _ in range(3):
                paced(k)
                k += 1
        arrange(None, False)
        for _ in range(args.prewarm):
            paced(k)
            k += 1
        times = {a[0]: [] for a in ARRANGEMENTS}
        for _ in range(args.rounds):
            for label, mx, gd in ARRANGEMENTS:
                arrange(mx, gd)
                times[label].append(block_ms(paced, args.steps, k))
                k += args.steps
        arrange(1.0, True)
        skipped, norm = opt.skipped_steps, float(opt.last_grad_norm)
        arrange(None, False)
        # the norm kernel alone, on this workload's gradient buffer
        n = opt.grad.numel()
        ctl, ws = opt._control(), opt._norm_ws
        norm_fn = lambda: ops.grad_norm(opt.grad, 2.0, ctl=ctl, ws=ws)
        ctrl_fn = lambda: ops.clip_control(ctl, 1.0, 1e-3, 0.9, 0.999, False)
        for _ in range(20):
            norm_fn()
            ctrl_fn()
        torch.cuda.synchronize()
        step_before = opt.step_count
        tn = [events_us(norm_fn, args.norm_reps) for _ in range(args.rounds)]
        tc = [events_us(ctrl_fn, args.norm_reps) for _ in range(args.rounds)]
        opt.step_count = step_before                                # (clip_control counted steps; nothing was applied)
        med = {k_: float(np.median(v)) for k_, v in times.items()}
        r3 = lambda x: round(float(x), 3)
        print(json.dumps({
            "workload": name, "flat_elements": n, "rounds": args.rounds, "steps_per_block": args.steps,
            "step_ms": {k_: {"median": r3(med[k_]), "min": r3(min(v)), "max": r3(max(v))} for k_, v in times.items()},
            "clip_minus_off_us": r3((med["clip"] - med["off"]) * 1e3), "guard_minus_off_us": r3((med["guard"] - med["off"]) * 1e3),
            "off_spread_us": r3((max(times["off"]) - min(times["off"])) * 1e3),
            "grad_norm_us": {"median": r3(np.median(tn)), "min": r3(min(tn)), "max": r3(max(tn))},
            "clip_control_us": {"median": r3(np.median(tc)), "min": r3(min(tc)), "max": r3(max(tc))},
            "hbm_floor_us_at_8000_GBs": r3(4 * n / bench.PEAK_HBM_GBS / 1e3), "hbm_floor_us_at_6290_GBs": r3(4 * n / HBM_COPY_GBS / 1e3),
            "grad_norm_over_floor_8000": r3(np.median(tn) / (4 * n / bench.PEAK_HBM_GBS / 1e3)),
            "achieved_GBs": r3(4 * n / np.median(tn) / 1e3),
            "skipped_steps": skipped, "last_grad_norm": norm}), flush=True)
        del ts, opt, paced
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
