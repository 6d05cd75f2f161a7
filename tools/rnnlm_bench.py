"""What the RNN language model costs, measured in one process by HIP events (alternating rounds, median and spread):

  * the kernels of lm.hip at the recipe's sizes -- embedding forward / backward (N = 40 960 and 102 400 ids over V = 62 rows of E = 128),
    NLL and the cross-entropy backward (N x 62 and 4 096 x 8 192), pack + select (B = 128, 10-best, T = 800) -- each beside the bytes it must
    move (`bytes`) and the rate they make;
  * one RNNLM training step (forward, loss, backward, FlatAdam) at V = 62, E = 128, H = 256, 2 LSTM layers, 32 sentences of 20 .. 60 phones;
  * BeamDecoder.decode on a 32 x 400 x 62 batch (W = 20, the golden bigram LM, peaky posteriors), plain and with 10-best RNN-LM rescoring,
    wall clock per batch including the copy to the host.

    python tools/rnnlm_bench.py [--reps 100] [--rounds 5] [--beam-reps 5]

One JSON line per measurement.  (DESIGN.md, section "RNN language model".)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_pytorch_amd import _lib, ops                               # noqa: E402
from ctc_pytorch_amd.testing import synth                          # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                          # us per call


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps                 # ms per call


def rounds(fns, n_rounds, reps, clock=timed):
    """{name: (median, min, max)} over n_rounds alternating rounds of `reps` calls each, after a warm-up of every function."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, fn in fns.items():
            out[k].append(clock(fn, reps))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in out.items()}


def report(what, stats, nbytes=None, **extra):
    med, lo, hi = stats
    line = dict(what=what, us=round(med, 2), us_min_max=[round(lo, 2), round(hi, 2)], **extra)
    if nbytes is not None:
        line.update(bytes=int(nbytes), gb_per_s=round(nbytes / med / 1e3, 1))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--beam-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rnnlm_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    L, P = _lib.lib(), _lib._ptr
    rng = np.random.RandomState(0)
    V, E = 62, 128

    table = torch.randn(V, E, device=dev)
    dtable = torch.zeros(V, E, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for N in (40960, 102400):
        ids = torch.from_numpy(rng.randint(0, V, size=N).astype(np.int32)).to(dev)
        y, dy = torch.empty(N, E, device=dev), torch.randn(N, E, device=dev)
        ws = torch.empty(L.ctcn_embedding_bwd_ws_bytes(N, V), dtype=torch.uint8, device=dev)
        fwd = lambda: L.ctcn_embedding_fwd(P(ids), P(table), P(y), N, V, E, -1, P(status), _lib.stream_ptr())
        bwd = lambda: L.ctcn_embedding_bwd(P(ids), P(dy), P(dtable), N, V, E, -1, 0.0, P(ws), ws.numel(), _lib.stream_ptr())
        r = rounds({"fwd": fwd, "bwd": bwd}, args.rounds, args.reps)
        report("embedding_fwd", r["fwd"], 4 * N + 4 * N * E + 4 * V * E, N=N, V=V, E=E)
        report("embedding_bwd", r["bwd"], 4 * N + 4 * N * E + 4 * V * E, N=N, V=V, E=E, rows_per_id=N // V, workspace_bytes=ws.numel())

    for N, Vx in ((40960, 62), (4096, 8192)):
        T, B = (N // 1024, 1024) if Vx == 62 else (N // 128, 128)
        lp = torch.log_softmax(torch.randn(N, Vx, device=dev), -1)
        tgt = torch.from_numpy(rng.randint(0, Vx, size=N).astype(np.int32)).to(dev)
        tok, sums = torch.empty(N, device=dev), torch.empty(B + 1, dtype=torch.float64, device=dev)
        count, dz, g = torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(N, Vx, device=dev), torch.ones(1, device=dev)
        nll = lambda: L.ctcn_nll_fwd(P(lp), P(tgt), T, B, Vx, -100, P(tok), P(sums), P(sums[B:]), P(count), P(status), _lib.stream_ptr())
        xb = lambda: L.ctcn_xent_bwd(P(lp), P(tgt), P(dz), N, Vx, -100, P(g), 0, P(count), _lib.stream_ptr())
        r = rounds({"nll": nll, "xent": xb}, args.rounds, args.reps)
        report("nll_fwd", r["nll"], 4 * N + 32 * N + 4 * N + 4 * N + 8 * B, N=N, V=Vx, T=T, B=B,
               note="bytes: targets, one 32-byte sector per gathered log-prob, tok written and read back, sums")
        report("xent_bwd", r["xent"], 8 * N * Vx + 4 * N, N=N, V=Vx, rows_by="wave" if Vx <= 512 else "workgroup")

    B, NB, T, Lh = 128, 10, 800, 60
    out_ids = torch.from_numpy(rng.randint(1, V, size=(B, NB, T)).astype(np.int32)).to(dev)
    out_len = torch.from_numpy(rng.randint(20, Lh + 1, size=(B, NB)).astype(np.int32)).to(dev)
    cnt = torch.full((B,), NB, dtype=torch.int32, device=dev)
    score, lm = -torch.rand(B, NB, dtype=torch.float64, device=dev), -30 * torch.rand(B, NB, dtype=torch.float64, device=dev)
    r = rounds({"pack": lambda: ops.pack_nbest(out_ids, out_len, cnt, Lh), "select": lambda: ops.rescore_select(score, lm, out_len, cnt, out_ids, 0.5, 0.0)},
               args.rounds, args.reps)
    report("lm_pack_nbest (with its three allocations)", r["pack"], 4 * B * NB * (2 * (Lh + 1) + 40 + 3), B=B, nbest=NB, T=T, L=Lh)
    report("rescore_select (with its four allocations)", r["select"], B * NB * 20 + B * (8 * T + 16), B=B, nbest=NB, T=T)

    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    from ctc_pytorch_amd.optim import FlatAdam
    torch.manual_seed(1)
    model = RNNLM(V, emb_size=E, hidden_size=256, layers=2, drop_out=0.1).to(dev)
    opt = FlatAdam(model, lr=1e-3)
    sents = [list(rng.randint(2, V, size=n)) for n in rng.randint(20, 61, size=32)]

    def step():
        loss = model.loss(sents, reduction="mean")
        opt.zero_grad()
        loss.backward()
        opt.step()
    r = rounds({"step": step}, args.rounds, max(args.reps // 5, 5), clock=wall)
    print(json.dumps({"what": "RNNLM training step", "ms": round(r["step"][0], 3), "ms_min_max": [round(r["step"][1], 3), round(r["step"][2], 3)],
                      "sentences": 32, "tokens": sum(len(s) + 1 for s in sents), "V": V, "E": E, "H": 256, "layers": 2}), flush=True)

    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    T, B, W = 400, 32, 20
    arpa = os.path.join(ROOT, "tests", "golden", "lm_phone_bg.arpa")
    plain = BeamDecoder(synth.int2char(V), beam_width=W, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.1)
    resc = BeamDecoder(synth.int2char(V), beam_width=W, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.1, rnnlm=model.eval(), rnnlm_nbest=10)
    lens = [int(v) for v in rng.randint(200, 401, size=B)]
    lp = torch.from_numpy(synth.make_logprobs(seed=7, T=T, B=B, V=V, regime="peaky")).to(dev)
    r = rounds({"plain": lambda: plain.decode(lp, lens), "rescored": lambda: resc.decode(lp, lens)}, args.rounds, args.beam_reps, clock=wall)
    best, _ = resc._rescored(lp, lens)
    print(json.dumps({"what": "BeamDecoder.decode", "T": T, "B": B, "V": V, "W": W, "nbest": 10, "longest_hypothesis": int(best.lengths.max()),
                      "plain_ms": round(r["plain"][0], 3), "plain_ms_min_max": [round(r["plain"][1], 3), round(r["plain"][2], 3)],
                      "rescored_ms": round(r["rescored"][0], 3), "rescored_ms_min_max": [round(r["rescored"][1], 3), round(r["rescored"][2], 3)],
                      "rescored_over_plain": round(r["rescored"][0] / r["plain"][0], 3)}), flush=True)


if __name__ == "__main__":
    main()
