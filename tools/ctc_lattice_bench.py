"""Time of the CTC lattice launch (ctcn_ctc_fwd_ex with beta: alpha and beta side by side, what nn.CTCLoss launches) with option
"ctc_lattice_skew" 0 (the classic kernels) and 1 (the wave-skewed kernel) on the same tensors in the same process, by HIP events, at the
lattice shapes of the workloads: cfg2 (T = 800, B = 32, V = 62, labels 30-60), cfg1 (300, 8, 62, 10-35), cfg4 (1200, 64, 200, 60-100) and the
shipped YAML (200, 8, 41, 20-40).  The yardstick is the classic kernel in the same session, not a number.

    python tools/ctc_lattice_bench.py [--reps 200] [--rounds 5]

Per shape: `--rounds` alternating rounds of `--reps` back-to-back launches under each option value after a warm-up of both; prints one JSON
line per shape with the median and the spread of the per-launch time over the rounds, the time per frame, the ratio of every round and
whether alpha, beta and nll of the two came out bit-identical.  """
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_pytorch_amd import _lib, ops                              # noqa: E402
from ctc_pytorch_amd.testing import synth                          # noqa: E402

SHAPES = (("cfg2", 800, 32, 62, 30, 60), ("cfg1", 300, 8, 62, 10, 35), ("cfg4", 1200, 64, 200, 60, 100), ("ref_yaml", 200, 8, 41, 20, 40))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ctc_lattice_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    default = ops.get_option("ctc_lattice_skew")
    for name, T, B, V, lo, hi in SHAPES:
        b = synth.make_batch(seed=1, B=B, T=T, F=4, V=V, lab_lo=lo, lab_hi=hi)
        lp = torch.from_numpy(synth.make_logprobs(2, T, B, V, "peaky")).to(dev)
        tg, il, tl = (torch.from_numpy(b[k]).to(dev) for k in ("targets", "lens", "tgt_len"))
        Lmax = tg.shape[1]
        s = _lib.stream_ptr()
        out = {}
        for skew in (0, 1):
            out[skew] = (torch.zeros((T, B, 2 * Lmax + 1), dtype=torch.float32, device=dev),
                         torch.zeros((T, B, 2 * Lmax + 1), dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev))

        def launch(skew):
            al, be, nl = out[skew]
            _lib.check(L.ctcn_ctc_fwd_ex(p(lp), p(tg), p(il), p(tl), p(al), p(be), p(nl), T, B, V, Lmax, 0, s), "ctc_fwd_ex")

        times = {0: [], 1: []}
        try:
            for skew in (0, 1):
                ops.set_option("ctc_lattice_skew", skew)
                plan = ops.ctc_lattice_plan(Lmax)
                for _ in range(20):
                    launch(skew)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for skew in (0, 1):
                    ops.set_option("ctc_lattice_skew", skew)
                    times[skew].append(timed(lambda: launch(skew), args.reps))
        finally:
            ops.set_option("ctc_lattice_skew", default)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out[0], out[1]))
        m0, m1 = float(np.median(times[0])), float(np.median(times[1]))
        print(json.dumps({"shape": name, "T": T, "B": B, "V": V, "Lmax": Lmax, "skewed_plan": plan,
                          "classic_us": round(m0, 2), "classic_us_min_max": [round(min(times[0]), 2), round(max(times[0]), 2)],
                          "skewed_us": round(m1, 2), "skewed_us_min_max": [round(min(times[1]), 2), round(max(times[1]), 2)],
                          "classic_us_per_frame": round(m0 / T, 4), "skewed_us_per_frame": round(m1 / T, 4),
                          "skewed_over_classic_per_round": [round(y / x, 3) for x, y in zip(times[0], times[1])],
                          "bit_identical": bool(same), "nll_finite": bool(torch.isfinite(out[1][2]).all())}), flush=True)


if __name__ == "__main__":
    main()
