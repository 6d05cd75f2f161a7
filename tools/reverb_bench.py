"""Time of reverberation and additive noise on the device (ctcn_reverb, the whole launch chain) by HIP events, at the recipe's waveform shape --
32 utterances of 8 s at 16 kHz, int16, ragged by a few frames as a length-sorted batch is -- against an impulse response of 800 taps (50 ms)
and one of 8 000 taps (0.5 s), each with and without a noise bank, normalisation on; and, as the yardsticks that this stage leaves
unchanged, ops.fbank and ops.resample (17 600 -> 16 000 Hz: speed 1.1) on the same audio.

    python tools/reverb_bench.py [--reps 20] [--rounds 5] [--yardsticks-only]

Per round, alternating: `--reps` back-to-back calls of each variant after a warm-up of all; prints one JSON line with the median and the
spread of the per-call time over the rounds and, for the reverberation, the two floors a result is judged against: the multiply-adds of the
full and the early-window convolution over the FP64 vector peak (78.6 TFLOP/s: half the FP32 vector rate), and the bytes the chain has to
move (the int16 batch read once, the float32 batch written once, read and written again by the noise and by the scaling launch, the noise
rows read once) over 6.29 TB/s, the measured HBM copy rate.  --yardsticks-only, or a tree without ops.reverberate, times the two yardsticks
alone: the same command, copied into a checkout of the parent commit, measures it like for like.  GPU only: no device, no number.
"""
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

FP64_VECTOR_FLOPS = 78.6e12
HBM_BYTES_PER_S = 6.29e12
FS = 16000


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


def impulse_response(K, rs):
    h = (rs.standard_normal(K) * np.exp(-np.arange(K) / (K / 5.0)) * 0.2).astype(np.float32)
    h[40] = 1.0
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--yardsticks-only", action="store_true", help="time ops.fbank and ops.resample alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "reverb_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    have = hasattr(ops, "reverberate") and not args.yardsticks_only
    rs = np.random.RandomState(0)
    B, N = 32, 8 * FS
    w16 = torch.from_numpy(np.clip(np.round(3000.0 * rs.standard_normal((B, N))), -32768, 32767).astype(np.int16)).to(dev)
    lens = [N - 160 * (b % 7) for b in range(B)]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    fns, floors = {}, {}
    if have:
        noises = [(rs.standard_normal(10 * FS) * 500.0).astype(np.float32) for _ in range(4)]
        for K in (800, 8000):
            h = impulse_response(K, rs)
            for with_noise in (False, True):
                bank = ops.ReverbBank([h], noises if with_noise else [], FS, device=dev)
                key = "reverberate_%d_taps%s_32x8s" % (K, "_noise" if with_noise else "")
                fns[key] = lambda bank=bank: ops.reverberate(w16, lens_d, bank, 1, 0)
                early = int(bank.rir_meta[0][3] - bank.rir_meta[0][2])
                # output i meets min(i + 1, K) taps; the early signal has n + E - 1 outputs, E of its taps meet min(i + 1, E, ...) samples: n E products
                fmas = sum(n * K - K * (K - 1) // 2 + n * early for n in lens)
                moved = sum(2 * n + 4 * n + 8 * n + (8 * n + 4 * n if with_noise else 0) for n in lens)
                floors[key] = {"fma": fmas, "bytes": moved, "fp64_floor_us": round(2 * fmas / FP64_VECTOR_FLOPS * 1e6, 1),
                               "hbm_floor_us": round(moved / HBM_BYTES_PER_S * 1e6, 1)}
    fb = features.Fbank(features.FbankConfig(window_type="hamming", num_mel_bins=80, use_energy=True, dither=0.0), dev)
    fns["fbank_int16_32x8s"] = lambda: ops.fbank(w16, lens, fb.plan)
    plan = ops.ResamplePlan(17600, FS)
    fns["resample_17600_16000_int16_32x8s"] = lambda: ops.resample(w16, lens, plan)
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    out = {"reverberate": have, "reps": args.reps, "rounds": args.rounds, "us_per_call": {k: spread(v) for k, v in times.items()}, "floors": floors}
    out["fp64_TFLOPs_at_median"] = {k: round(2 * floors[k]["fma"] / (out["us_per_call"][k]["median"] * 1e-6) / 1e12, 2) for k in floors}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
