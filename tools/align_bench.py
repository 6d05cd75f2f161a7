"""Time of ctcn_ctc_align beside the alpha-only loss forward (ctcn_ctc_fwd_ex with beta = NULL) on the same tensors in the same process, by HIP
events: cfg2's shape (T = 800, B = 32, V = 62, synth labels) and a decode-sized batch (B = 128).  The yardstick is the existing kernel, not a
number: the alignment chain does a max where the loss does a log-sum-exp, and adds a trace of T dependent LDS reads.

    python tools/align_bench.py [--reps 200] [--rounds 5]
    CTCN_LIBCTCN=<library built with -DCTCN_ALIGN_FORWARD_ONLY> python tools/align_bench.py --forward-only      # phase split

Per shape: `--rounds` alternating rounds of `--reps` back-to-back launches of each kernel after a warm-up of both; prints the median and the
spread of the per-launch time over the rounds and their ratio, one JSON line per shape.  """
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_pytorch_amd import _lib                                   # noqa: E402
from ctc_pytorch_amd.testing import synth                          # noqa: E402


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
    ap.add_argument("--forward-only", action="store_true",
                    help="the loaded library (CTCN_LIBCTCN) was built with -DCTCN_ALIGN_FORWARD_ONLY: its alignment kernel stops after the forward "
                         "chain, so ctc_align_us is the fills + the chain and the difference to the product build is the trace + output phase")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "align_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for name, B in (("cfg2", 32), ("decode_batch", 128)):
        T, V = 800, 62
        b = synth.make_batch(seed=1, B=B, T=T, F=4, V=V, lab_lo=30, lab_hi=60)
        lp = torch.from_numpy(synth.make_logprobs(2, T, B, V, "peaky")).to(dev)
        tg, il, tl = (torch.from_numpy(b[k]).to(dev) for k in ("targets", "lens", "tgt_len"))
        Lmax = tg.shape[1]
        alpha = torch.empty((T, B, 2 * Lmax + 1), dtype=torch.float32, device=dev)
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        paths = torch.empty((B, T), dtype=torch.int32, device=dev)
        fs = torch.empty((B, T), dtype=torch.float32, device=dev)
        sc, ok = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        st, en = torch.empty((B, Lmax), dtype=torch.int32, device=dev), torch.empty((B, Lmax), dtype=torch.int32, device=dev)
        need = L.ctcn_ctc_align_ws_bytes(T, B, Lmax)
        ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
        s = _lib.stream_ptr()

        def fwd():
            _lib.check(L.ctcn_ctc_fwd_ex(p(lp), p(tg), p(il), p(tl), p(alpha), None, p(nll), T, B, V, Lmax, 0, s), "ctc_fwd_ex")

        def align():
            _lib.check(L.ctcn_ctc_align(p(lp), p(tg), p(il), p(tl), p(paths), p(fs), p(sc), p(ok), p(st), p(en), T, B, V, Lmax, 0, p(ws), need, s),
                       "ctc_align")

        for _ in range(20):
            fwd()
            align()
        torch.cuda.synchronize()
        tf, ta = [], []
        for _ in range(args.rounds):
            tf.append(timed(fwd, args.reps))
            ta.append(timed(align, args.reps))
        assert bool(ok.all()) and bool(torch.isfinite(nll).all())
        assert args.forward_only or bool((paths[:, 0] >= 0).all())
        mf, ma = float(np.median(tf)), float(np.median(ta))
        print(json.dumps({"shape": name, "forward_only_build": args.forward_only, "T": T, "B": B, "V": V, "Lmax": Lmax, "rows_in_lds": need == 0,
                          "ctc_fwd_alpha_only_us": round(mf, 2), "ctc_fwd_alpha_only_us_min_max": [round(min(tf), 2), round(max(tf), 2)],
                          "ctc_align_us": round(ma, 2), "ctc_align_us_min_max": [round(min(ta), 2), round(max(ta), 2)],
                          "align_over_fwd": round(ma / mf, 3)}), flush=True)


if __name__ == "__main__":
    main()
