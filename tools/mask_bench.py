"""What the length-aware forward / backward (CTC_Model.forward(input_lengths=)) costs and saves per training step, and the masked
BatchNorm against the bytes it has to move.

    python tools/mask_bench.py [--workloads cfg2] [--rounds 5] [--steps 20] [--prewarm 40]

Per workload, in ONE process, one model / optimiser, the step of bench.make_training_step (forward -> CTC / B -> backward -> FlatAdam.step,
paced two steps ahead) with the model called in four arrangements, timed in `--rounds` alternating rounds of `--steps` steps (host clock
around a block that ends in a device synchronise) after `--prewarm` untimed steps:
    full_off     full-length batch, no lengths                  (the unmasked step: what bench.py's headline times)
    full_on      the same batch, input_lengths = [T] * B        (a) the price of the feature
    ragged_off   lengths U{T/4 .. T} (bench.py's epoch_loop_ragged draw), zero-padded, no lengths
    ragged_on    the same batch, input_lengths given            (b) what skipping the padded rows saves
Then the BatchNorm of one recurrent layer alone (rows layout, T*B x 2H: forward-train + backward, HIP events around back-to-back calls):
unmasked, masked with full lengths, masked with the ragged lengths, beside the bytes the masked passes have to move
(forward: 2 reads + 1 write of the valid elements; backward with no ReLU: x and dy twice + dx = 5; the zeros of the padded rows are written
too) at the measured float4-copy rate.  One JSON line per workload.  (DESIGN.md, section on length-aware masking.)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                       # noqa: E402
from ctc_pytorch_amd import nn, ops                                # noqa: E402
from ctc_pytorch_amd.optim import FlatAdam                         # noqa: E402
from ctc_pytorch_amd.testing import synth                          # noqa: E402

HBM_COPY_GBS = 6290.0                                              # measured float4 copy on the MI355X


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
    ap.add_argument("--workloads", default="cfg2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--prewarm", type=int, default=bench.PREWARM)
    ap.add_argument("--bn-reps", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mask_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    for name in args.workloads.split(","):
        c = bench.WORKLOADS[name]
        B, T, Fd = c["B"], c["T"], c.get("F", 40)
        torch.manual_seed(1)
        model = bench.build(c, dev, drop_out=c.get("drop", 0.1)).train()
        opt = FlatAdam(model, lr=1e-3, weight_decay=5e-4)
        loss_fn = nn.CTCLoss(reduction="sum")
        full = synth.make_batch(seed=1, B=B, T=T, F=Fd, V=c["V"], lab_lo=c["lab"][0], lab_hi=c["lab"][1], full_length=True)
        rs = np.random.RandomState(11)
        rag_lens = np.array([int(rs.randint(T // 4, T + 1)) for _ in range(B)], dtype=np.int64)
        rag_lens[0] = T
        xr = full["x"].copy()
        for b in range(B):
            xr[b, rag_lens[b]:] = 0.0
        out_full = model.output_lengths(np.full(B, T, dtype=np.int64))
        out_rag = model.output_lengths(rag_lens)
        tl_rag = np.minimum(full["tgt_len"], np.maximum(1, out_rag.numpy() // 3))
        tg = torch.from_numpy(full["targets"]).to(dev)

        def arrangement(x, lens, out_len, tl, masked):
            xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)          # lengths resident like the batch
            in_len, tld = out_len.to(dev), torch.from_numpy(tl).to(dev)

            def step():
                out = model(xd, input_lengths=ld) if masked else model(xd)
                loss = loss_fn(out, tg, in_len, tld) / B
                opt.zero_grad()
                loss.backward()
                ops.join_side_stream()
                opt.step()
            return step

        full_lens = np.full(B, T, dtype=np.int64)
        steps = {"full_off": arrangement(full["x"], full_lens, out_full, full["tgt_len"], False),
                 "full_on": arrangement(full["x"], full_lens, out_full, full["tgt_len"], True),
                 "ragged_off": arrangement(xr, rag_lens, out_rag, tl_rag, False),
                 "ragged_on": arrangement(xr, rag_lens, out_rag, tl_rag, True)}
        ring = [torch.cuda.Event() for _ in range(3)]
        k = [0]

        def paced(fn):
            fn()
            ring[k[0] % 3].record()
            if k[0] >= 2:
                ring[(k[0] - 2) % 3].synchronize()
            k[0] += 1

        def block_ms(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                paced(fn)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps

        for fn in steps.values():
            for _ in range(3):
                paced(fn)
        for _ in range(args.prewarm):
            paced(steps["full_off"])
        times = {label: [] for label in steps}
        for _ in range(args.rounds):
            for label, fn in steps.items():
                times[label].append(block_ms(fn))
        kernels = ops.rnn_last_kernels()
        ops.check_health()
        med = {label: float(np.median(v)) for label, v in times.items()}

        # one recurrent layer's BatchNorm alone: rows layout, T' * B x 2H
        Tp, C = int(out_full[0]), 2 * c["H"]
        rows = Tp * B
        x = torch.randn(rows, C, device=dev)
        dy = torch.randn(rows, C, device=dev)
        gamma, beta = torch.ones(C, device=dev, requires_grad=True), torch.zeros(C, device=dev, requires_grad=True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        lens_full = torch.full((B,), Tp, dtype=torch.int32, device=dev)
        lens_rag = out_rag.to(torch.int32).to(dev)

        def bn(lengths):
            xin = x.detach().requires_grad_(True)

            def fwd():
                return ops.batch_norm(xin, gamma, beta, rm, rv, rows, C, 1, True, lengths=lengths)

            def both():
                fwd().backward(dy)
            for _ in range(10):
                both()
            torch.cuda.synchronize()
            with torch.no_grad():
                f = [events_us(fwd, args.bn_reps) for _ in range(args.rounds)]
            t = [events_us(both, args.bn_reps) for _ in range(args.rounds)]
            return float(np.median(f)), float(np.median(t)) - float(np.median(f))

        bn_us = {"unmasked": bn(None), "masked_full": bn(lens_full), "masked_ragged": bn(lens_rag)}
        valid = int(out_rag.sum()) * C
        total = rows * C
        r3 = lambda v: round(float(v), 3)
        bytes_fwd = lambda n: 4 * (2 * n + total)                    # two reads of the valid elements, y written everywhere
        bytes_bwd = lambda n: 4 * (4 * n + total)                    # x and dy twice (valid), dx written everywhere
        print(json.dumps({
            "workload": name, "rounds": args.rounds, "steps_per_block": args.steps, "rnn_kernels": kernels,
            "ragged_valid_share": r3(float(rag_lens.sum()) / (B * T)),
            "step_ms": {label: {"median": r3(med[label]), "min": r3(min(v)), "max": r3(max(v))} for label, v in times.items()},
            "full_on_minus_off_us": r3((med["full_on"] - med["full_off"]) * 1e3),
            "full_off_spread_us": r3((max(times["full_off"]) - min(times["full_off"])) * 1e3),
            "ragged_on_minus_off_us": r3((med["ragged_on"] - med["ragged_off"]) * 1e3),
            "ragged_off_spread_us": r3((max(times["ragged_off"]) - min(times["ragged_off"])) * 1e3),
            "bn_layer": {"rows": rows, "C": C, "valid_elements_ragged": valid, "elements": total,
                         "fwd_bwd_us": {label: {"fwd": r3(v[0]), "bwd": r3(v[1])} for label, v in bn_us.items()},
                         "masked_ragged_bytes": {"fwd": bytes_fwd(valid), "bwd": bytes_bwd(valid), "four_valid_passes_fwd": 4 * valid * 3, "four_valid_passes_bwd": 4 * valid * 5},
                         "masked_ragged_floor_us_at_6290_GBs": {"fwd": r3(bytes_fwd(valid) / HBM_COPY_GBS / 1e3), "bwd": r3(bytes_bwd(valid) / HBM_COPY_GBS / 1e3)},
                         "unmasked_floor_us_at_6290_GBs": {"fwd": r3(4 * 3 * total / HBM_COPY_GBS / 1e3), "bwd": r3(4 * 5 * total / HBM_COPY_GBS / 1e3)}},
        }), flush=True)
        del model, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
