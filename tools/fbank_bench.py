"""Time of the filterbank front-end (ctcn_fbank) on a cfg2-like batch -- 32 utterances x 8 s of 16 kHz audio, the reference's shipped
fbank.conf (hamming, 80 bins, energy: 81 dimensions) -- by HIP events, with and without the fused normalisation, and of
ctcn_cmvn_accumulate on its output; beside it the float32 numpy restatement (tests/fbank_ref.py) on the host's threads.

    python tools/fbank_bench.py [--reps 50] [--rounds 5] [--batch 32] [--seconds 8] [--cpu-threads 16] [--mfcc] [--spectrogram] [--logspec]
                                [--resample]

--mfcc adds ctcn_mfcc on the same batch to the alternating rounds of the same process: Kaldi's MFCC defaults (23 bins, 13 cepstra) and 80
bins / 64 cepstra under the filterbank leg's frame options, and ctcn_fbank with the MFCC defaults' 23 bins.

--spectrogram adds ctcn_spectrogram (Kaldi's defaults: 257 columns, three times the filterbank's output) with and without the fused
normalisation; --logspec adds ctcn_logspec (the recipe's 400-point STFT, 201 columns) raw and normalised -- the normalisation reads and
writes its output once more, which its algorithmic bytes count.

--resample adds ctcn_resample on the same int16 batch read at 14400, 17600 (speed factors 0.9 and 1.1) and 44100 Hz, each to 16 kHz, and
the chain resample + filterbank (0.9: the float32 output fed to ctcn_fbank with its lengths); beside the bytes, the LDS reads the sums
need (two 4-byte reads per tap and lane) and the float32 numpy restatement of the three pairs on the host's threads.

Per round, alternating: `--reps` back-to-back launches of each variant after a warm-up of all; prints one JSON line with the median and
the spread of the per-call time over the rounds, the bytes the algorithm has to move (bytes(wave) + 4 F T B) and the rate that makes of
the median, and the host figure (wall clock, one pass over the same batch, utterances dealt to a thread pool).  GPU only: no device, no
number.  """
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fbank_ref                                                   # noqa: E402
import resample_ref                                                # noqa: E402
from ctc_pytorch_amd import ops                                    # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--mfcc", action="store_true", help="time ops.mfcc next to ops.fbank in the same rounds")
    ap.add_argument("--spectrogram", action="store_true", help="time ops.spectrogram (Kaldi's defaults) in the same rounds")
    ap.add_argument("--logspec", action="store_true", help="time ops.log_spectrum (the recipe's defaults), raw and normalised, in the same rounds")
    ap.add_argument("--resample", action="store_true", help="time ops.resample (14400, 17600, 44100 -> 16000 Hz) and resample + fbank in the same rounds")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fbank_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    kw = dict(window_type="hamming", num_mel_bins=80, use_energy=True, dither=0.0)
    fb = features.Fbank(features.FbankConfig(**kw), dev)
    B, N = args.batch, int(args.seconds * 16000)
    rs = np.random.RandomState(0)
    host = np.clip(np.round(3000.0 * rs.standard_normal((B, N))), -32768, 32767).astype(np.int16)
    lens = [N - 160 * (b % 7) for b in range(B)]                   # ragged by a few frames, as a length-sorted batch is
    w16 = torch.from_numpy(host).to(dev)
    w32 = w16.to(torch.float32)
    F, T = fb.feat_dim, fb.num_frames(N)
    mean = torch.full((F,), 15.0, device=dev)
    scale = torch.full((F,), 0.25, device=dev)
    feats, frames = ops.fbank(w16, lens, fb.plan)
    stats = torch.zeros((2, F + 1), dtype=torch.float64, device=dev)
    fns = {
        "fbank_int16": lambda: ops.fbank(w16, lens, fb.plan),
        "fbank_int16_normalised": lambda: ops.fbank(w16, lens, fb.plan, mean=mean, scale=scale),
        "fbank_float32": lambda: ops.fbank(w32, lens, fb.plan),
        "cmvn_accumulate": lambda: ops.cmvn_accumulate(feats, frames, stats),
    }
    algo_extra = {}
    if args.mfcc:
        for key, mkw in (("mfcc_int16_defaults", dict()), ("mfcc_int16_80bins_64ceps", dict(window_type="hamming", num_mel_bins=80, num_ceps=64))):
            mf = features.Mfcc(features.MfccConfig(dither=0.0, **mkw), dev)
            fns[key] = lambda plan=mf.plan: ops.mfcc(w16, lens, plan)
            algo_extra[key] = 2 * B * N + 4 * mf.feat_dim * T * B
        # the filterbank of the MFCC defaults' frame and mel options (povey, 23 bins, energy): what stages 1-4 cost there
        fb23 = features.Fbank(features.FbankConfig(dither=0.0, use_energy=True), dev)
        fns["fbank_int16_23bins"] = lambda: ops.fbank(w16, lens, fb23.plan)
        algo_extra["fbank_int16_23bins"] = 2 * B * N + 4 * fb23.feat_dim * T * B
    if args.spectrogram:
        sp = features.Spectrogram(features.SpectrogramConfig(dither=0.0), dev)
        smean, sscale = torch.full((sp.feat_dim,), 15.0, device=dev), torch.full((sp.feat_dim,), 0.25, device=dev)
        fns["spectrogram_int16"] = lambda: ops.spectrogram(w16, lens, sp.plan)
        fns["spectrogram_int16_normalised"] = lambda: ops.spectrogram(w16, lens, sp.plan, mean=smean, scale=sscale)
        algo_extra["spectrogram_int16"] = algo_extra["spectrogram_int16_normalised"] = 2 * B * N + 4 * sp.feat_dim * sp.num_frames(N) * B
    if args.logspec:
        for key, normalize in (("logspec_int16_raw", False), ("logspec_int16_normalised", True)):
            ls = features.LogSpectrum(features.LogSpecConfig(normalize=normalize), dev)
            fns[key] = lambda plan=ls.plan: ops.log_spectrum(w16, lens, plan)
            out_bytes = 4 * ls.feat_dim * ls.num_frames(N) * B
            algo_extra[key] = 2 * B * N + out_bytes * (3 if normalize else 1)       # normalised: written, read and written again
    lds_reads = {}
    if args.resample:
        plans = {fin: ops.ResamplePlan(fin, 16000) for fin in (14400, 17600, 44100)}
        for fin, plan in plans.items():
            key = "resample_int16_%d_16000" % fin
            fns[key] = lambda plan=plan: ops.resample(w16, lens, plan)
            outs = [plan.num_samples(n) for n in lens]
            algo_extra[key] = 2 * sum(lens) + 4 * B * max(outs)                     # the samples once, the padded output once
            lds_reads[key] = 8 * int(sum((m // plan.ou) * int(plan.ntaps.sum()) + int(plan.ntaps[:m % plan.ou].sum()) for m in outs))

        def chain(plan=plans[14400]):
            w, wl = ops.resample(w16, lens, plan)
            return ops.fbank(w, wl, fb.plan)
        fns["resample_14400_16000_then_fbank"] = chain
        m09 = plans[14400].num_samples(N)
        algo_extra["resample_14400_16000_then_fbank"] = algo_extra["resample_int16_14400_16000"] + 4 * B * m09 + 4 * F * fb.num_frames(m09) * B
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    out = {"batch": B, "samples": N, "frames": T, "feat_dim": F, "reps": args.reps, "rounds": args.rounds,
           "us_per_call": {k: spread(v) for k, v in times.items()}}
    # what the algorithm has to move: the samples once, the features once (ops.fbank also uploads B lengths and allocates its outputs: part of the call)
    algo = {"fbank_int16": 2 * B * N + 4 * F * T * B, "fbank_int16_normalised": 2 * B * N + 4 * F * T * B, "fbank_float32": 4 * B * N + 4 * F * T * B,
            "cmvn_accumulate": 4 * F * T * B}
    algo.update(algo_extra)
    out["algorithmic_bytes"] = algo
    out["algorithmic_GBps_at_median"] = {k: round(algo[k] / (out["us_per_call"][k]["median"] * 1e-6) / 1e9, 1) for k in algo}
    if lds_reads:
        out["resample_lds_read_bytes"] = lds_reads
        out["resample_lds_read_TBps_at_median"] = {k: round(v / (out["us_per_call"][k]["median"] * 1e-6) / 1e12, 2) for k, v in lds_reads.items()}
    if args.resample and not args.no_cpu:
        cpu = {}
        with ThreadPoolExecutor(max_workers=args.cpu_threads) as pool:
            for fin, plan in plans.items():
                one = lambda b: resample_ref.resample(host[b, :lens[b]], fin, 16000, plan.first, plan.ntaps, plan.weights)
                list(pool.map(one, range(min(B, args.cpu_threads))))                 # warm-up
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(one, range(B)))
                    ts.append((time.perf_counter() - t0) * 1e6)
                cpu["resample_int16_%d_16000" % fin] = spread(ts)
        out["cpu_resample_restatement_us"] = dict(cpu, threads=args.cpu_threads)
    if not args.no_cpu:
        o = fbank_ref.options(**kw)
        waves = [host[b, :lens[b]].astype(np.float32) for b in range(B)]
        cpu = []
        with ThreadPoolExecutor(max_workers=args.cpu_threads) as pool:
            list(pool.map(lambda w: fbank_ref.fbank(w, o, np.float32), waves[:args.cpu_threads]))      # warm-up
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(lambda w: fbank_ref.fbank(w, o, np.float32), waves))
                cpu.append((time.perf_counter() - t0) * 1e6)
        out["cpu_float32_restatement_us"] = dict(spread(cpu), threads=args.cpu_threads)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
