"""Time of the pitch front-end on a cfg2-like batch -- 32 utterances x 8 s of 16 kHz audio, Kaldi's defaults (417 lags, three columns) -- by
HIP events: the downsampling (ctcn_resample to 4 kHz), the extraction (ctcn_pitch: sums, correlation and upsampling, Viterbi and walk
back), the post-processing (ctcn_pitch_process) and the whole utils/features.Pitch call; beside them the unchanged neighbours (ctcn_fbank
on the same batch, ctcn_resample 14400 -> 16000) so that a run at another commit can be laid next to this one, and the numpy restatement
(tests/pitch_ref.py: float64 extraction, float32 post-processing) on the host's threads.

    python tools/pitch_bench.py [--reps 20] [--rounds 5] [--batch 32] [--seconds 8] [--cpu-threads 16] [--no-cpu] [--neighbours-only]

Per round, alternating: `--reps` back-to-back calls of each variant after a warm-up of all; prints one JSON line with the median and the
spread of the per-call time over the rounds, the Viterbi's share per frame and utterance where the kernels are timed one by one (run the
tool under a kernel trace for that: the three kernels of ctcn_pitch are pitch_var_kernel, pitch_nccf_kernel, pitch_viterbi_kernel), and
the floors of the correlation phase: its float64 operations (6 per sample, lag and frame, plus 2 per tap, lag and frame) and the bytes it
has to move (the samples once, two float32 planes of S values per frame once).  GPU only: no device, no number.  
--neighbours-only: the filterbank and the resampler alone -- what a checkout without the pitch front-end can run."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--neighbours-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pitch_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    B, N = args.batch, int(args.seconds * 16000)
    rs = np.random.RandomState(0)
    t = np.arange(N) / 16000.0
    host = np.stack([3000.0 * np.sin(2 * np.pi * (90.0 + 9.0 * b) * t) + 1500.0 * np.sin(2 * np.pi * 2 * (90.0 + 9.0 * b) * t)
                     + 800.0 * rs.standard_normal(N) for b in range(B)])
    host = np.clip(np.round(host), -32768, 32767).astype(np.int16)
    lens = [N - 160 * (b % 7) for b in range(B)]                   # ragged by a few frames, as a length-sorted batch is
    w16 = torch.from_numpy(host).to(dev)
    fb = features.Fbank(features.FbankConfig(window_type="hamming", num_mel_bins=80, use_energy=True, dither=0.0), dev)
    rplan = ops.ResamplePlan(14400, 16000)
    fns = {"fbank_int16": lambda: ops.fbank(w16, lens, fb.plan), "resample_int16_14400_16000": lambda: ops.resample(w16, lens, rplan)}
    out = {"batch": B, "samples": N, "reps": args.reps, "rounds": args.rounds}
    if not args.neighbours_only:
        import ctypes
        from ctc_pytorch_amd import _lib
        pitch = features.Pitch(device=dev)
        plan = pitch.plan
        S, T = plan.num_lags, plan.num_frames(N)
        down, dlens = ops.resample(w16, lens, plan.resample_plan)
        raw, frames = ops.pitch(w16, lens, plan)
        L, p = _lib.lib(), lambda x: ctypes.c_void_p(x.data_ptr())
        dl = torch.as_tensor(dlens, dtype=torch.int32).to(dev)
        ws = _lib.workspace(dev, nbytes=L.ctcn_pitch_workspace_bytes(ctypes.byref(plan.opts), B, T), tag="pitch")

        def extract():
            _lib.check(L.ctcn_pitch(p(down), p(dl), ctypes.byref(plan.opts), p(plan.on(dev)), p(raw), None, p(frames), B, down.shape[1], T, p(ws),
                                    ws.numel(), _lib.stream_ptr()), "pitch")
        fns.update({"downsample_16000_4000": lambda: ops.resample(w16, lens, plan.resample_plan), "extract_downsampled": extract,
                    "process": lambda: ops.pitch_process(raw, frames), "pitch_whole_call": lambda: pitch(w16, lens)})
        nm, W, taps = plan.last_lag - plan.first_lag + 1, plan.window, int(plan.tap_count.sum())
        frames_total = int(frames.sum().item())
        out.update({"frames": T, "frames_total": frames_total, "lags": S, "measured_lags": nm,
                    "correlation_fp64_ops": frames_total * (6 * W * nm + 2 * 2 * taps),
                    "correlation_bytes": 4 * sum(dlens) + 2 * 4 * S * frames_total,
                    "viterbi_pairs": frames_total * S * S})
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    out["us_per_call"] = {k: spread(v) for k, v in times.items()}
    if not args.neighbours_only:
        out["extract_us_per_frame_of_an_utterance_at_median"] = round(out["us_per_call"]["extract_downsampled"]["median"] / T, 3)
        if not args.no_cpu:
            import pitch_ref
            rp = pitch_ref.Plan()
            one = lambda b: pitch_ref.process(pitch_ref.extract(rp, host[b, :lens[b]])[0], np.float32)
            with ThreadPoolExecutor(max_workers=args.cpu_threads) as pool:
                t0 = time.perf_counter()
                list(pool.map(one, range(B)))
                out["cpu_restatement_us"] = {"one_pass": round((time.perf_counter() - t0) * 1e6), "threads": args.cpu_threads}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
