"""What timed, scored output costs over plain decoding, measured in one process:

  * ctcn_path_tokens beside ctcn_argmax + ctcn_greedy_collapse -- all that GreedyDecoder.decode launches -- on the same tensors at cfg2's shape
    (T = 800, B = 32, V = 62, peaky posteriors, lens U{400..800}), by HIP events, alternating rounds;
  * BeamDecoder.decode_timed beside BeamDecoder.decode at cfg5 (W = 20, the golden bigram LM, alpha 0.1, 128 x 800 x 62, both regimes), wall
    clock per batch including the copy to the host and the host-side assembly, one batch at a time.

    python tools/path_tokens_bench.py [--reps 200] [--rounds 5] [--beam-reps 10]

One JSON line per measurement; `lp_bytes` is 4 T B V, `bytes_read` what the kernel read of it.  """
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_pytorch_amd import ops                                    # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--beam-reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "path_tokens_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")

    T, B, V = 800, 32, 62
    lp = torch.from_numpy(synth.make_logprobs(2, T, B, V, "peaky")).to(dev)
    lens = torch.from_numpy(np.random.RandomState(2).randint(400, 801, size=B).astype(np.int32)).to(dev)
    idx = ops.argmax_last(lp)
    plain = lambda: ops.greedy_collapse(ops.argmax_last(lp), lens, blank=0)
    tokens = lambda: ops.path_tokens(idx, lens, lp, blank=0)
    both = lambda: ops.path_tokens(ops.argmax_last(lp), lens, lp, blank=0)
    for _ in range(20):
        plain(), tokens(), both()
    torch.cuda.synchronize()
    tp, tt, tb = [], [], []
    for _ in range(args.rounds):
        tp.append(timed(plain, args.reps))
        tt.append(timed(tokens, args.reps))
        tb.append(timed(both, args.reps))
    pt = tokens()
    ids, n = plain()
    assert torch.equal(pt.lengths, n)
    frames = int(lens.sum())
    in_token = int((pt.ends - pt.starts)[pt.starts >= 0].sum())
    mp, mt, mb = (float(np.median(v)) for v in (tp, tt, tb))
    print(json.dumps({"shape": "cfg2", "T": T, "B": B, "V": V, "frames": frames, "frames_in_tokens": in_token, "tokens": int(n.sum()),
                      "argmax_plus_greedy_collapse_us": round(mp, 2), "argmax_plus_greedy_collapse_us_min_max": [round(min(tp), 2), round(max(tp), 2)],
                      "path_tokens_us": round(mt, 2), "path_tokens_us_min_max": [round(min(tt), 2), round(max(tt), 2)],
                      "argmax_plus_path_tokens_us": round(mb, 2), "timed_over_plain": round(mb / mp, 3),
                      "lp_bytes": 4 * T * B * V, "bytes_read": 4 * (in_token * V + (frames - in_token)) + 16 * frames,
                      "bytes_written": 4 * (6 * B * T + 2 * B)}), flush=True)

    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    T, B, W = 800, 128, 20
    dec = BeamDecoder(synth.int2char(V), beam_width=W, blank_index=0, space_idx=-1, lm_path=os.path.join(ROOT, "tests", "golden", "lm_phone_bg.arpa"),
                      lm_alpha=0.1)
    lens = [int(v) for v in np.random.RandomState(2).randint(400, 801, size=B)]
    for regime in ("peaky", "flat"):
        lp = torch.from_numpy(synth.make_logprobs(seed=7, T=T, B=B, V=V, regime=regime)).to(dev)
        strings, timed_out = dec.decode(lp, lens), dec.decode_timed(lp, lens)
        assert [" ".join(t[0] for t in e[0]) for e in timed_out] == strings
        td, tt = [], []
        for _ in range(args.rounds):
            td.append(wall(lambda: dec.decode(lp, lens), args.beam_reps))
            tt.append(wall(lambda: dec.decode_timed(lp, lens), args.beam_reps))
        md, mt = float(np.median(td)), float(np.median(tt))
        print(json.dumps({"shape": "cfg5", "regime": regime, "T": T, "B": B, "V": V, "W": W, "tokens": sum(len(e[0]) for e in timed_out),
                          "longest_hypothesis": max(len(e[0]) for e in timed_out),
                          "decode_ms": round(md, 3), "decode_ms_min_max": [round(min(td), 3), round(max(td), 3)],
                          "decode_timed_ms": round(mt, 3), "decode_timed_ms_min_max": [round(min(tt), 3), round(max(tt), 3)],
                          "timed_over_plain": round(mt / md, 3)}), flush=True)


if __name__ == "__main__":
    main()
