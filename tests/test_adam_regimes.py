"""adam_kernel and adam_ex_kernel (csrc/elementwise.hip) against float64, where eps and the bias corrections decide.

test_adam_vs_oracle compares three steps on N(0,1) gradients under max|p - p_ref| < 2e-6: about 1e-3 of an update, with |g| ~ 1, where
eps = 1e-8 is invisible and the bias corrections are those of the first steps.  Real gradients span 1e-10 .. 1e-2 and hold exact zeros.
Here (tests/adam_ref.py; tests/test_adam_regimes_host.py holds the reference to torch.optim.Adam in float64 and shows that a float32 replay
of the kernels' expression meets the bounds):

1. The SWEEP: single steps from a designed state of n = 4099 elements (one odd tail; the buffers 16-byte aligned and, again, 4-byte aligned
   only) -- g in {0, +-2^k}, k = -60 .. 40, on a 12-bit grid; v in {0, 2^k}, k = -120 .. 80; m at matching scales; p in {0, +-1e-3, +-1, +-1e4}
   -- under every (step, lr, weight decay) of adam_ref.sweep_calls.  ops.adam_step directly; ops.clip_control + ops.adam_step_ex with a control
   block at clip_coef 1 (then bit for bit ops.adam_step's where step_size and sqrt_bc2 agree) and about 0.1, and with apply = 0 (nothing
   written, bit for bit).  p', m', v' within the per-element bounds DERIVED in adam_ref.bounds from the kernels' expression; step_size and
   sqrt_bc2 of the control block within one float32 rounding of the float64 expressions.

2. 200 steps, n = 10007, gradients log-uniform in magnitude over 1e-10 .. 1e-2 with 5 % exact zeros, lr 1e-3, weight decay 5e-4.  The gate is
   MEASURED, not derived: torch's float32 CPU Adam against the float64 reference on the same data ends at
       max|p - p_ref| / (lr * steps) = 1.309e-5      (max|p - p_ref| = 2.62e-6; the float32 replay of the kernels' expression: the same figure)
   and the kernel is allowed 4x that, 5.24e-5: both sides accumulate the same kind of rounding, and neither is the code under test.

CTCN_REGIME_LOG=<file>: one JSON line per call with max(error / bound) per output.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu
TORCH_F32_MULTI_STEP = 1.309e-5          # measured (module docstring); the gate is 4x this
MODES = ("step", "ex_clip1", "ex_clip0.1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _log(record):
    path = os.environ.get("CTCN_REGIME_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def _buffers(s, dev, offset):
    """p, g, m, v on the device at `offset` floats past a 16-byte boundary"""
    out = {}
    for k in "pgmv":
        buf = torch.zeros(s[k].size + offset, device=dev)
        out[k] = buf[offset:]
        out[k].copy_(torch.from_numpy(s[k].copy()))
        assert out[k].data_ptr() % 16 == 4 * offset
    return out


def _control(dev, ops, t, lr, total_norm, nonfinite=0, skip=False):
    """a control block as ctcn_grad_norm would leave it (total_norm, nonfinite), through ctcn_clip_control with max_norm 1"""
    ctl = ops.new_clip_ctl(dev, step=t - 1)
    ctl.view(torch.float32)[ops.CTL_NORM] = total_norm
    ctl[ops.CTL_NONFINITE] = nonfinite
    ops.clip_control(ctl, 1.0, lr, A.B1, A.B2, skip_nonfinite=skip)
    return ctl


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("t,lr,wd", A.sweep_calls())
def test_sweep_single_steps_within_bounds(dev, t, lr, wd, offset):
    from ctc_pytorch_amd import ops
    s = A.sweep_state()
    got, ctl_words, rec = {}, {}, {"test": "adam", "step": t, "lr": lr, "wd": wd, "offset": offset}
    for mode in MODES:
        d = _buffers(s, dev, offset)
        clip = 1.0
        if mode == "step":
            ops.adam_step(d["p"], d["g"], d["m"], d["v"], lr, A.B1, A.B2, A.EPS, wd, t)
        else:
            ctl = _control(dev, ops, t, lr, 0.5 if mode == "ex_clip1" else 10.0)
            ops.adam_step_ex(d["p"], d["g"], d["m"], d["v"], A.B1, A.B2, A.EPS, wd, ctl)
            c = ctl.cpu()
            cf = c.view(torch.float32)
            clip, ss, sbc = float(cf[ops.CTL_COEF]), float(cf[ops.CTL_STEP_SIZE]), float(cf[ops.CTL_SQRT_BC2])
            assert int(c[ops.CTL_APPLY]) == 1 and int(c[ops.CTL_STEP]) == t and int(c[ops.CTL_SKIPPED]) == 0
            assert clip == 1.0 if mode == "ex_clip1" else abs(clip - 0.1) < 1e-6           # (the reference takes the block's own float32 value)
            ctl_words[mode] = (ss, sbc)
            want_ss, want_sbc = A.corrections(t, lr)
            # one float32 rounding each (u), on a float64 expression whose pow is good to a few 2^-53
            assert abs(ss - want_ss) <= (A.U + 2.0 ** -48) * want_ss and abs(sbc - want_sbc) <= (A.U + 2.0 ** -48) * want_sbc, (ss, want_ss, sbc, want_sbc)
            rec[mode + " step_size"], rec[mode + " sqrt_bc2"] = abs(ss - want_ss) / (A.U * want_ss), abs(sbc - want_sbc) / (A.U * want_sbc)
        assert torch.equal(d["g"], torch.from_numpy(s["g"].copy()).to(dev))                 # the gradient is never written
        ref = A.step(s["p"], s["g"], s["m"], s["v"], t, lr, wd, clip)
        bnd = A.bounds(s["p"], s["g"], s["m"], s["v"], t, lr, wd, clip)
        got[mode] = {k: d[k].cpu().numpy() for k in "pmv"}
        for k, r in zip("pmv", ref):
            a = got[mode][k].astype(np.float64)
            assert np.all(np.isfinite(a)), (mode, k)
            err = np.abs(a - r)
            rec["%s %s" % (mode, k)] = A.ratio(err, bnd[k])
            assert np.all(err <= bnd[k]), (mode, k, rec["%s %s" % (mode, k)], int(np.argmax(err / bnd[k])))
    # clip_coef = 1: adam_kernel's bits, where the device's pow and the host's gave the same float32 step_size and sqrt_bc2 (include/ctcn.h)
    if ctl_words["ex_clip1"] == tuple(float(np.float32(x)) for x in A.corrections(t, lr)):
        for k in "pmv":
            assert np.array_equal(got["ex_clip1"][k], got["step"][k]), k
        rec["ex_clip1 bitwise"] = 1
    # apply = 0: a non-finite norm under skip_nonfinite drops the step -- nothing is written, the step count stays
    d = _buffers(s, dev, offset)
    ctl = _control(dev, ops, t, lr, float("inf"), nonfinite=1, skip=True)
    ops.adam_step_ex(d["p"], d["g"], d["m"], d["v"], A.B1, A.B2, A.EPS, wd, ctl)
    c = ctl.cpu()
    assert int(c[ops.CTL_APPLY]) == 0 and int(c[ops.CTL_STEP]) == t - 1 and int(c[ops.CTL_SKIPPED]) == 1
    for k in "pgmv":
        assert np.array_equal(d[k].cpu().numpy().view(np.int32), s[k].view(np.int32)), k
    _log(rec)


_multi = []


@pytest.mark.parametrize("mode", ["step", "ex"])
def test_two_hundred_steps_on_log_uniform_gradients(dev, mode):
    """Module docstring, point 2: torch's float32 CPU Adam ends at 1.309e-5 (in units of lr * steps) from the float64 reference; the kernel is
    allowed 4x that = 5.24e-5."""
    from ctc_pytorch_amd import ops
    lr, wd = A.f32v(1e-3), A.f32v(5e-4)
    if not _multi:                                           # computed once, shared by the two modes, never written to
        p0, gs = A.multi_step_data()
        _multi.extend([p0, gs, A.multi_step_reference(p0, gs, lr, wd)])
    p0, gs, ref = _multi
    n = p0.size
    p, m, v = torch.from_numpy(p0.copy()).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    gd = torch.from_numpy(np.stack(gs)).to(dev)
    ctl = ops.new_clip_ctl(dev)
    ctl.view(torch.float32)[ops.CTL_NORM] = 0.5              # below max_norm = 1: clip_coef 1 at every step
    for t in range(1, len(gs) + 1):
        if mode == "step":
            ops.adam_step(p, gd[t - 1], m, v, lr, A.B1, A.B2, A.EPS, wd, t)
        else:
            ops.clip_control(ctl, 1.0, lr, A.B1, A.B2)
            ops.adam_step_ex(p, gd[t - 1], m, v, A.B1, A.B2, A.EPS, wd, ctl)
    got = p.cpu().numpy().astype(np.float64)
    assert mode == "step" or int(ctl.cpu()[ops.CTL_STEP]) == len(gs)
    figure = float(np.max(np.abs(got - ref)) / (lr * len(gs)))
    _log({"test": "adam_multi", "mode": mode, "figure": figure, "torch_f32": TORCH_F32_MULTI_STEP})
    print("\n[adam %s] max|p - p_ref| / (lr * steps) = %.3e (torch float32 on the CPU: %.3e)" % (mode, figure, TORCH_F32_MULTI_STEP))
    assert np.all(np.isfinite(got)) and figure <= 4 * TORCH_F32_MULTI_STEP, figure
