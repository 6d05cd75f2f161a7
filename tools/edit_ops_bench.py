"""Time of ctcn_edit_ops beside ctcn_edit_distance on the same tensors in the same process, by HIP events, and of a validation pass of
steps/train_ctc.run_epoch with the error report off and on.

    python tools/edit_ops_bench.py [--reps 200] [--rounds 5] [--no-epoch]
    CTCN_LIBCTCN=<library built with -DCTCN_EDIT_OPS_FORWARD_ONLY> python tools/edit_ops_bench.py --forward-only --no-epoch     # phase split

Kernels: cfg2's scoring shape, 32 x (800 x <= 60 labels), with two kinds of hypotheses -- "trained" (the label with a fifth of its symbols
substituted, dropped or doubled: what a validation pass late in training scores) and "untrained" (the greedy collapse of random peaky
posteriors: a few hundred symbols against <= 60).  Per case `--rounds` alternating rounds of `--reps` back-to-back launches of the distance
kernel, the breakdown counts-only, and the breakdown with pairs and table, after a warm-up of all three; prints the median and the spread of
the per-launch time over the rounds, one JSON line per case.  The yardstick is the existing kernel, not a number.
Epoch: a cfg2 model (bench.build), 6 device-resident batches, run_epoch(is_training=False) with error_report off / on / on with a score map,
alternating, wall clock around the pass (it ends with the host having read the last step's statistics).  """
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctc_pytorch_amd import _lib, ops                              # noqa: E402
from ctc_pytorch_amd.testing import synth                          # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                          # us per launch


def spread(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(float(min(xs)), 2), "max": round(float(max(xs)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--forward-only", action="store_true",
                    help="the loaded library (CTCN_LIBCTCN) was built with -DCTCN_EDIT_OPS_FORWARD_ONLY: its kernel stops before the walk, so the "
                         "breakdown's time is staging + recursion + move stores and the difference to the product build is the walk + outputs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "edit_ops_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    B, T, V = 32, 800, 62
    b = synth.make_batch(seed=1, B=B, T=T, F=4, V=V, lab_lo=30, lab_hi=60)
    tg, tl = torch.from_numpy(b["targets"]).to(dev), torch.from_numpy(b["tgt_len"]).to(dev)
    ldb = tg.shape[1]
    rs = np.random.RandomState(3)
    trained = np.zeros((B, T), dtype=np.int32)
    trained_len = np.zeros(B, dtype=np.int32)
    for u in range(B):
        out = []
        for k in b["targets"][u, :b["tgt_len"][u]]:
            r = rs.rand()
            out += [] if r < 0.07 else [int(rs.randint(1, V))] if r < 0.14 else [int(k), int(k)] if r < 0.2 else [int(k)]
        trained[u, :len(out)], trained_len[u] = out, len(out)
    lp = torch.from_numpy(synth.make_logprobs(2, T, B, V, "peaky")).to(dev)
    un_ids, un_len = ops.greedy_collapse(ops.argmax_last(lp), torch.full((B,), T, dtype=torch.int32, device=dev), blank=0)
    cases = {"trained": (torch.from_numpy(trained).to(dev), torch.from_numpy(trained_len).to(dev)), "untrained": (un_ids, un_len)}
    dist = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty((B, 6), dtype=torch.int32, device=dev)
    ali = torch.empty((B, T + ldb, 2), dtype=torch.int32, device=dev)
    ali_len = torch.empty(B, dtype=torch.int32, device=dev)
    conf = torch.zeros((V + 1, V + 1), dtype=torch.int64, device=dev)
    assert L.ctcn_edit_ops_ws_bytes(B, T, ldb) == 0
    s = _lib.stream_ptr()
    for name, (ids, idl) in cases.items():
        fns = {
            "edit_distance_us": lambda: L.ctcn_edit_distance(p(ids), p(idl), p(tg), p(tl), p(dist), B, T, ldb, ldb, s),
            "edit_ops_counts_us": lambda: L.ctcn_edit_ops(p(ids), p(idl), p(tg), p(tl), None, 0, p(counts), None, None, None, B, T, ldb, ldb, None, 0, s),
            "edit_ops_pairs_table_us": lambda: L.ctcn_edit_ops(p(ids), p(idl), p(tg), p(tl), None, V, p(counts), p(ali), p(ali_len), p(conf), B, T, ldb,
                                                               ldb, None, 0, s),
        }
        for fn in fns.values():
            assert fn() == 0
            timed(fn, 20)
        if not args.forward_only:
            assert torch.equal(counts[:, :3].sum(1, dtype=torch.int32), dist)
        rounds = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, args.reps))
        line = {"case": name, "B": B, "lda": T, "ldb": ldb, "mean_hyp_len": round(float(idl.float().mean()), 1), "mean_ref_len": round(float(tl.float().mean()), 1),
                "forward_only": bool(args.forward_only)}
        line.update({k: spread(v) for k, v in rounds.items()})
        print(json.dumps(line), flush=True)
    if args.no_epoch or args.forward_only:
        return
    import bench
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.steps.train_ctc import run_epoch
    c = bench.WORKLOADS["cfg2"]
    model = bench.build(c, dev, 0.1)
    loss_fn = nn.CTCLoss(reduction="sum")
    eb = synth.make_batch(seed=0, B=c["B"], T=c["T"], F=40, V=c["V"], lab_lo=c["lab"][0], lab_hi=c["lab"][1])
    data = [(torch.from_numpy(eb["x"]).to(dev), torch.ones(c["B"], device=dev), torch.from_numpy(eb["targets"]).to(dev),
             torch.from_numpy(eb["tgt_len"]).to(dev), None)] * 6
    cmap = np.arange(c["V"], dtype=np.int32)
    cmap[5], cmap[7] = 4, -1
    modes = {"valid_epoch_off_ms": {}, "valid_epoch_report_ms": {"error_report": True}, "valid_epoch_report_map_ms": {"error_report": True, "score_map": cmap}}
    times = {k: [] for k in modes}
    for r in range(args.rounds + 1):
        for k, kw in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_epoch(0, model, data, loss_fn, dev, is_training=False, log=lambda *_: None, **kw)
            torch.cuda.synchronize()
            if r:                                                  # round 0 warms up
                times[k].append(1e3 * (time.perf_counter() - t0) / len(data))
    print(json.dumps(dict({"case": "cfg2 validation pass, ms per batch", "batches": len(data)}, **{k: spread(v) for k, v in times.items()})), flush=True)


if __name__ == "__main__":
    main()
