"""The float64 Adam reference, the sweep and its derived bounds, checked without a GPU (no gpu marker).

tests/test_adam_regimes.py holds adam_kernel and adam_ex_kernel to tests/adam_ref.py on single steps from designed states.  Checked here:
  * the reference is torch.optim.Adam in float64 on the CPU, to 1e-12 of the terms each result is formed from (m' = b1 m + (1 - b1) g' may
    cancel, and torch forms it as a lerp: the two agree relative to |b1 m| + |(1 - b1) g'|, not to m')
  * the float32 replay of the kernels' expression stays inside the bounds on every call of the sweep -- the reference alone satisfies the
    gates.  Measured, the largest error / bound: p' 1.00 (p' = p where the step is below half an ulp of p: u |p'| is bound and error),
    m' 0.89, v' 0.87.  torch's own float32 Adam is logged next to it (CTCN_REGIME_LOG; no gate: it forms m' as a lerp and the step with
    addcdiv, another rounding sequence) and stays inside the same bounds: p' 1.00, m' 0.80, v' 0.87.
  * the sweep reaches where eps sits: elements with sqrt(v') < eps (the denominator IS eps), within a factor 4 of eps, and beyond 1e6 eps
  * the bias corrections: at step 1 000, 1 - beta1^t differs from 1 by less than 1e-6 and 1 - beta2^t by more than 1e-5 (0.37), and at 10 000
    still by 4.5e-5; at step 100 000 BOTH are 1 to float64 resolution (0.999^100000 = 4e-44) -- the sweep keeps that step for the large
    exponent of pow, and 10 000 (added to the five of the issue) for a large step at which beta2's correction still acts.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as A  # noqa: E402

CLIPS = (1.0, float(np.float32(1.0) / (np.float32(10.0) + np.float32(1e-6))))


def _log(record):
    path = os.environ.get("CTCN_REGIME_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def _torch_adam(s, t, lr, wd, dtype):
    p = torch.nn.Parameter(torch.tensor(s["p"], dtype=dtype))
    p.grad = torch.tensor(s["g"], dtype=dtype)
    opt = torch.optim.Adam([p], lr=lr, betas=(A.B1, A.B2), eps=A.EPS, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(s["m"], dtype=dtype), "exp_avg_sq": torch.tensor(s["v"], dtype=dtype)}
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t
    return tuple(a.detach().double().numpy() for a in (p, st["exp_avg"], st["exp_avg_sq"]))


@pytest.mark.parametrize("t,lr,wd", A.sweep_calls())
def test_reference_is_torch_adam_in_float64(t, lr, wd):
    s = A.sweep_state()
    p1, m1, v1 = A.step(s["p"], s["g"], s["m"], s["v"], t, lr, wd)
    tp, tm, tv = _torch_adam(s, t, lr, wd, torch.float64)
    g1 = s["g"].astype(np.float64) + wd * s["p"].astype(np.float64)
    terms = np.abs(A.B1 * s["m"].astype(np.float64)) + np.abs((1 - A.B1) * g1)
    ss, sbc = A.corrections(t, lr)
    d = np.sqrt(v1) / sbc + A.EPS
    assert np.all(np.abs(tm - m1) <= 1e-12 * terms)
    assert np.all(np.abs(tv - v1) <= 1e-12 * v1)
    assert np.all(np.abs(tp - p1) <= 1e-12 * (np.abs(s["p"]) + ss * terms / d))


@pytest.mark.parametrize("clip", CLIPS, ids=["clip1", "clip0.1"])
@pytest.mark.parametrize("t,lr,wd", A.sweep_calls())
def test_replay_stays_inside_the_bounds(t, lr, wd, clip):
    s = A.sweep_state()
    ref = A.step(s["p"], s["g"], s["m"], s["v"], t, lr, wd, clip)
    got = A.replay(s["p"], s["g"], s["m"], s["v"], t, lr, wd, clip)
    bnd = A.bounds(s["p"], s["g"], s["m"], s["v"], t, lr, wd, clip)
    rec = {"test": "adam_host", "step": t, "lr": lr, "wd": wd, "clip": clip}
    for k, a, b in zip("pmv", got, ref):
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), k
        err = np.abs(a - b)
        assert np.all(err <= bnd[k]), (k, A.ratio(err, bnd[k]))
        rec["replay " + k] = A.ratio(err, bnd[k])
    if clip == 1.0:
        for k, a, b in zip("pmv", _torch_adam(s, t, lr, wd, torch.float32), ref):
            rec["torch_f32 " + k] = A.ratio(np.abs(a - b), bnd[k])
    _log(rec)


def test_sweep_reaches_where_eps_sits():
    s = A.sweep_state()
    for k in "pgmv":
        assert s[k].size == A.N and A.N % 4 == 3
    assert np.sum(s["g"] == 0) > 100 and np.sum(s["v"] == 0) > 100 and np.sum(s["m"] == 0) > 100
    g = np.abs(s["g"][s["g"] != 0].astype(np.float64))
    assert g.min() < 2.0 ** -55 and g.max() > 2.0 ** 36 and np.all(np.round(g / 2.0 ** np.floor(np.log2(g)) * 2 ** 11) == g / 2.0 ** np.floor(np.log2(g)) * 2 ** 11)
    v = s["v"][s["v"] != 0].astype(np.float64)
    assert v.min() < 2.0 ** -110 and v.max() > 2.0 ** 70
    assert set(np.unique(s["p"])) == set(np.float32(x) for x in A.P_VALUES)
    for t, lr, wd in A.sweep_calls():
        _, _, v1 = A.step(s["p"], s["g"], s["m"], s["v"], t, lr, wd)
        r = np.sqrt(v1)
        # (with weight decay only the elements with p = 0, one in seven, keep a g' below eps)
        assert np.sum(r < A.EPS) >= 50 and np.sum((r > A.EPS / 4) & (r < 4 * A.EPS)) >= 50 and np.sum(r > 1e6 * A.EPS) > 1000, (t, lr, wd)
        assert np.sum(v1 == 0) > 0


def test_bias_corrections_at_large_steps():
    b1t, b2t = (lambda t: A.B1 ** t), (lambda t: A.B2 ** t)
    assert b1t(1000) < 1e-6 and b2t(1000) > 1e-5
    assert b1t(10000) < 1e-6 and b2t(10000) > 1e-5
    assert b1t(100000) < 1e-6 and b2t(100000) < 1e-40          # not "more than 1e-5": 0.999^100000 = 4e-44
    assert set(A.STEPS) >= {1, 2, 10, 1000, 100000}
