"""What trigram LM scoring costs in the beam search, by HIP events, on the cfg5 batch (128 x 800 x 62, peaky and flat posteriors, lens
U{400..800}, the golden bigram LM at alpha 0.1) at W = 20 (the fast kernel) and W = 200 (the generic kernel), alternating rounds in one
process:

  * order2          ctcn_beam_decode as shipped (W = 20: alpha * LM in LDS);
  * order2_global   the same with beam_occ2 = 2, the fast kernel's build that reads the LM from global memory (two workgroups per CU; the
                    generic kernel at W = 200 already reads it from global memory next to its 97-KB candidate table: the option changes nothing there);
  * order3          ctcn_beam_decode_lm with a context-free (V+1)^3 table (tri[c0] = the bigram table: the same search, bit for bit,
                    so the legs differ by the table read alone), and under beam_occ2 = 2 as order3_occ2;
  * parent_order2   ctcn_beam_decode of another build of the library (--parent-lib: libctcn.so of the parent commit), same process,
                    same buffers.

    python tools/beam_trigram_bench.py [--reps 10] [--rounds 7] [--parent-lib PATH]

One JSON line per (regime, W): median, min and max of the rounds in ms per batch.  ("Trigram LM scoring".)"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctc_pytorch_amd import _lib, ops                              # noqa: E402
from ctc_pytorch_amd.testing import synth                          # noqa: E402
from ctc_pytorch_amd.utils.NgramLM import LanguageModel            # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps                                # ms per call


class Search(object):
    """One library's beam entry on preallocated buffers (no allocation, no copy inside the timed region)."""

    def __init__(self, lib, x, lens, W):
        self.lib, self.x, self.lens, self.W = lib, x, lens, W
        T, B, V = x.shape
        dev = x.device
        lib.ctcn_beam_ws_bytes.restype = ctypes.c_size_t
        self.ws = torch.empty(max(lib.ctcn_beam_ws_bytes(T, B, V, W), 1), dtype=torch.uint8, device=dev)
        self.ids = torch.zeros((B, T), dtype=torch.int32, device=dev)
        self.len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.score = torch.zeros(B, dtype=torch.float64, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)

    def __call__(self, lm, alpha, order=2):
        T, B, V = self.x.shape
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        common = (P(self.ids), P(self.len), P(self.score))
        tail = (P(self.status), T, B, V, P(self.ws), ctypes.c_size_t(self.ws.numel()), st)
        if order == 2:
            rc = self.lib.ctcn_beam_decode(P(self.x), 0, P(self.lens), P(lm), ctypes.c_double(alpha), self.W, 0, *common, *tail)
        else:
            rc = self.lib.ctcn_beam_decode_lm(P(self.x), 0, P(self.lens), P(lm), order, ctypes.c_double(alpha), self.W, 0, 1, *common, None, *tail)
        assert rc == 0, rc

    def result(self):
        torch.cuda.synchronize()
        return self.ids.cpu().numpy().copy(), self.len.cpu().numpy().copy(), self.score.cpu().numpy().copy(), self.status.cpu().numpy().copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="libctcn.so built from the parent commit (leg parent_order2)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "beam_trigram_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    T, B, V, alpha = 800, 128, 62, 0.1
    i2c = synth.int2char(V)
    lm2_h = LanguageModel(os.path.join(ROOT, "tests", "golden", "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
    lm2 = torch.from_numpy(lm2_h).to(dev)
    lm3 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(lm2_h, (V + 1,) * 3))).to(dev)
    lens = torch.from_numpy(np.random.RandomState(2).randint(400, 801, size=B).astype(np.int32)).to(dev)
    parent = ctypes.CDLL(args.parent_lib) if args.parent_lib else None
    for regime in ("peaky", "flat"):
        x = torch.from_numpy(synth.make_logprobs(seed=7, T=T, B=B, V=V, regime=regime)).to(dev)
        for W in (20, 200):
            here = Search(_lib.lib(), x, lens, W)
            legs = {"order2": lambda: here(lm2, alpha), "order2_global": lambda: (ops.set_option("beam_occ2", 2), here(lm2, alpha), ops.set_option("beam_occ2", 0)),
                    "order3": lambda: here(lm3, alpha, 3),
                    "order3_occ2": lambda: (ops.set_option("beam_occ2", 2), here(lm3, alpha, 3), ops.set_option("beam_occ2", 0))}
            if parent is not None:
                there = Search(parent, x, lens, W)
                legs["parent_order2"] = lambda: there(lm2, alpha)
            want = None
            for name, fn in legs.items():                              # warm-up, and every leg returns the same search
                fn()
                got = (there if name == "parent_order2" else here).result()
                want = want or got
                assert all(np.array_equal(u, v) for u, v in zip(got, want)), name
            times = {name: [] for name in legs}
            for _ in range(args.rounds):
                for name, fn in legs.items():
                    times[name].append(timed(fn, args.reps))
            row = {"regime": regime, "T": T, "B": B, "V": V, "W": W, "path": ops.beam_plan(T, B, V, W)["path"],
                   "path_order3": ops.beam_plan(T, B, V, W, lm_order=3)["path"], "reps": args.reps, "rounds": args.rounds}
            for name, v in times.items():
                row[name + "_ms"] = round(float(np.median(v)), 3)
                row[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
