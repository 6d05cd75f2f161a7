"""The float64 reference of the recurrent layer and the trained-model regimes, checked without a GPU (no gpu marker).

tests/test_rnn_regimes.py holds the seven recurrence kernels of rnn.hip to tests/rnn_cell_ref.py outside the linear regime.  That only
means something if (1) the reference is right, (2) each regime really is what it says -- saturated, long-lived, not chaotic -- at every
shape the GPU tests use, and (3) the activations' 3e-7 claim is reachable by the formula at all.  Those are checked here.

Measured (the conditions are asserted; these are the figures behind them).  Per case: share of gate pre-activations with |a| > 4, then
torch float32 against torch float64: max|dy| and the worst rel-L2 of dx and the weight gradients; `memory`: median forget / update gate, max|c|.

  cell regime   T,  B,  I,  H  dirs  |a|>4   y         gradients
  lstm input16 48,  5,  8,  32 x2    0.36   5.2e-07   3.6e-07
  lstm input64 48,  5,  8,  32 x2    0.81   1.2e-06   5.8e-07
  lstm mixed   48,  5,  8,  32 x2    0.21   2.9e-07   3.4e-07
  lstm memory  48,  5,  8,  32 x2    0.18   2.5e-07   5.8e-07   keep 0.995  |c| 33.2
  gru  input16 48,  5,  8,  32 x2    0.38   6.3e-07   3.4e-07
  gru  input64 48,  5,  8,  32 x2    0.82   1.5e-06   5.2e-07
  gru  mixed   48,  5,  8,  32 x2    0.16   6.6e-07   3.6e-07
  gru  memory  48,  5,  8,  32 x2    0.22   2.6e-07   2.6e-06   keep 0.992
  lstm input16 48, 17, 16,  72 x2    0.35   6.7e-07   3.7e-07
  lstm input64 48, 17, 16,  72 x2    0.81   2.4e-06   7.7e-07
  lstm mixed   48, 17, 16,  72 x2    0.19   1.2e-06   5.2e-07
  lstm memory  48, 17, 16,  72 x2    0.17   6.8e-07   4.9e-07   keep 0.995  |c| 40.4
  gru  input16 48, 17, 16,  72 x2    0.35   9.9e-07   3.9e-07
  gru  input64 48, 17, 16,  72 x2    0.81   3.1e-06   7.0e-07
  gru  mixed   48, 17, 16,  72 x2    0.17   1.7e-06   4.0e-07
  gru  memory  48, 17, 16,  72 x2    0.24   2.7e-07   3.6e-06   keep 0.995
  lstm input16 24,  9, 16, 320 x2    0.06   5.3e-07   3.4e-07
  lstm input64 24,  9, 16, 320 x2    0.62   1.3e-06   4.6e-07
  lstm mixed   24,  9, 16, 320 x2    0.08   9.3e-07   3.7e-07
  lstm memory  24,  9, 16, 320 x2    0.16   4.5e-07   5.4e-07   keep 0.993  |c| 15.0
  gru  input16 24,  9, 16, 320 x2    0.06   5.9e-07   3.5e-07
  gru  input64 24,  9, 16, 320 x2    0.62   2.5e-06   4.4e-07
  gru  mixed   24,  9, 16, 320 x2    0.08   1.0e-06   3.8e-07
  gru  memory  24,  9, 16, 320 x2    0.23   1.3e-07   3.2e-06   keep 0.994
  lstm input16 24,  9, 16, 384 x2    0.03   4.3e-07   3.9e-07
  lstm input64 24,  9, 16, 384 x2    0.59   1.8e-06   4.6e-07
  lstm mixed   24,  9, 16, 384 x2    0.07   4.3e-07   4.2e-07
  lstm memory  24,  9, 16, 384 x2    0.17   5.3e-07   6.2e-07   keep 0.993  |c| 14.3
  gru  input16 24,  9, 16, 384 x2    0.04   6.7e-07   4.0e-07
  gru  input64 24,  9, 16, 384 x2    0.60   2.3e-06   4.7e-07
  gru  mixed   24,  9, 16, 384 x2    0.07   8.2e-07   4.1e-07
  gru  memory  24,  9, 16, 384 x2    0.22   1.3e-07   3.4e-06   keep 0.992
  lstm input16 12, 33,  8, 512 x2    0.00   1.9e-07   3.7e-07
  lstm input64 12, 33,  8, 512 x2    0.38   7.9e-07   3.8e-07
  lstm mixed   12, 33, 32, 512 x2    0.10   8.2e-07   4.7e-07   (I = 8 gives 0.03: below the regime's 0.05, rnn_cell_ref.MIXED_WIDE)
  lstm memory  12, 33,  8, 512 x2    0.16   2.3e-07   6.1e-07   keep 0.992  |c| 5.3
  gru  input16 12, 33,  8, 512 x2    0.00   3.4e-07   3.5e-07
  gru  input64 12, 33,  8, 512 x2    0.38   7.8e-07   3.7e-07
  gru  mixed   12, 33, 32, 512 x2    0.10   1.4e-06   4.5e-07
  gru  memory  12, 33,  8, 512 x2    0.22   7.1e-08   2.5e-06   keep 0.993
  tanh input16 48,  5,  8,  32 x2    0.38   7.1e-07   3.1e-07
  tanh input64 48,  5,  8,  32 x2    0.82   2.5e-06   6.0e-07
  tanh mixed   48,  5,  8,  32 x2    0.18   1.5e-06   3.7e-07
  tanh input16 48, 17, 16,  72 x2    0.36   1.1e-06   3.4e-07
  tanh input64 48, 17, 16,  72 x2    0.82   3.4e-06   7.1e-07
  tanh mixed   48, 17, 16,  72 x2    0.19   2.3e-06   3.6e-07
  lstm mixed   48,  5,  8,  32 x1    0.15   4.5e-07   3.1e-07
  gru  memory  48, 17, 16,  72 x1    0.21   2.7e-07   3.1e-06   keep 0.989
  lstm memory  12,144, 16, 320 x2    0.17   4.2e-07   5.0e-07   keep 0.993  |c| 8.2
Worst: y 3.4e-6 (cap 4e-6), gradients 3.6e-6 (cap 5e-6).  The GRU in `memory` with a per-utterance input offset (as the LSTM has it) sits
at 4.9-5.5e-6 on dx and is not used (rnn_cell_ref, regime comment).
The float32 restatement of the two activation formulas, exp2 and the reciprocal each an ulp either way, on every argument of the sweep:
sigmoid <= 1.4e-7, tanh <= 1.6e-7 from float64 (claim: 3e-7), finite everywhere.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnn_cell_ref as R  # noqa: E402

CASES = R.layer_cases()
_id = lambda k: "%s-%s-T%dB%dI%dH%dx%d" % k


@pytest.fixture(scope="module")
def torch_f64():
    """torch's own layer in float64 per case: computed once, shared by the reference test and the no-chaos condition"""
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = R.torch_layer(key[0], R.layer_case(key)[0], torch.float64)
        return cache[key]
    return get


def _rel_max(a, b):
    return R.max_abs(a, b) / max(float(np.max(np.abs(b))), 1e-300)


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_reference_equals_torch_double(key, torch_f64):
    """forward and backward, all three cells, one and two directions, every regime: 1e-12 relative (of the tensor's largest magnitude)"""
    _, ref = R.layer_case(key)
    want = torch_f64(key)
    assert _rel_max(ref["y"], want["y"]) <= 1e-12
    for (name, got), (_, w) in zip(R.gradients(ref), R.gradients(want)):
        assert _rel_max(got, w) <= 1e-12, name


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_regime_meets_its_condition(key, torch_f64):
    """Conditions, not measurements: a shape or seed that misses one is replaced, the caps stay (the GPU gates rest on them)."""
    cell, regime, T, B, I, H, dirs = key
    case, ref = R.layer_case(key)
    share = R.saturated_share(ref["pre"])
    f32, f64 = R.torch_layer(cell, case, torch.float32), torch_f64(key)
    dy_, dg_ = R.max_abs(f32["y"], f64["y"]), max(R.rel_l2(a, b) for (_, a), (_, b) in zip(R.gradients(f32), R.gradients(f64)))
    line = "%-34s |a|>4: %.2f  torch f32 vs f64: y %.1e  gradients %.1e" % (_id(key), share, dy_, dg_)
    if regime == "input64":
        assert share >= 0.30, line
    if regime == "mixed":
        assert share >= 0.05, line
    if regime == "memory":
        keep = ref["act"][..., H:2 * H]                      # block 1: the forget (LSTM) / update (GRU) gate
        line += "  median keep gate %.3f" % float(np.median(keep))
        assert np.median(keep) >= 0.9, line
        if cell == "lstm":
            line += "  max|c| %.1f" % float(np.max(np.abs(ref["aux"])))
            assert np.max(np.abs(ref["aux"])) >= 3.0, line
    print(line)
    # no chaos: torch's own float32 layer stays next to its float64 self
    assert dy_ <= 4e-6, line
    assert dg_ <= 5e-6, line


# ---- the activation formulas of rnn.hip, restated in numpy float32 -----------------------------------------------------------------
f32 = np.float32


def _ulp_step(v, k):
    """v moved k ulps (k in -1, 0, 1); infinities and zeros stay"""
    v = np.asarray(v, dtype=f32)
    if k == 0:
        return v
    moved = np.nextafter(v, f32(np.inf if k > 0 else -np.inf))
    return np.where(np.isfinite(v) & (v != 0), moved, v).astype(f32)


def _exp2(v, k):
    with np.errstate(over="ignore", under="ignore"):
        return _ulp_step(np.exp2(v.astype(np.float64)).astype(f32), k)


def _rcp(v, k):
    with np.errstate(divide="ignore", over="ignore"):
        return _ulp_step((1.0 / v.astype(np.float64)).astype(f32), k)


def sigmoid_f32(x, ke, kr):
    """act_sigmoid: rcp(1 + exp2(-log2(e) * x)), every operation rounded to float32"""
    with np.errstate(over="ignore"):
        return _rcp(f32(1.0) + _exp2(f32(-1.4426950408889634) * x, ke), kr)


def tanh_f32(x, ke, kr):
    """act_tanh: copysign((1 - e) * rcp(1 + e), x) with e = exp2(-2 log2(e) |x|)"""
    with np.errstate(over="ignore"):
        e = _exp2(f32(-2.8853900817779268) * np.abs(x), ke)
    return np.copysign((f32(1.0) - e) * _rcp(f32(1.0) + e, kr), x).astype(f32)


@pytest.mark.parametrize("ke", [-1, 0, 1])
@pytest.mark.parametrize("kr", [-1, 0, 1])
def test_activation_formulas_reach_their_claim_in_float32(ke, kr):
    """|error| < 3e-7 absolute (the comment above act_sigmoid) with exp2 and the reciprocal each off by one ulp either way, on every
    pre-activation of the sweep; finite everywhere; the hard edges come out exact."""
    a = R.sweep_arguments().astype(f32)
    assert a.size > 200 and np.all(np.isfinite(a))
    s, t = sigmoid_f32(a, ke, kr), tanh_f32(a, ke, kr)
    assert s.dtype == f32 and t.dtype == f32 and np.all(np.isfinite(s)) and np.all(np.isfinite(t))
    es, et = R.max_abs(s, R.sigmoid(a.astype(np.float64))), R.max_abs(t, np.tanh(a.astype(np.float64)))
    print("exp2 %+d ulp, rcp %+d ulp: sigmoid %.2e  tanh %.2e" % (ke, kr, es, et))
    assert es < 3e-7 and et < 3e-7
    if ke == 0 and kr == 0:                       # a reciprocal that is an ulp off cannot return exactly 1
        big = np.abs(a) >= 1000
        assert np.array_equal(s[big], (a[big] > 0).astype(f32))
        sat = np.abs(a) >= 16
        assert np.array_equal(t[sat], np.sign(a[sat]).astype(f32))
    zeros = tanh_f32(np.array([0.0, -0.0], dtype=f32), ke, kr)
    assert not np.signbit(zeros[0]) and np.signbit(zeros[1])                    # -0 stays -0
    if ke == 0:                                   # (exp2(0) is exactly 1; moved by an ulp it is not, and 1 - e is that ulp)
        assert np.all(zeros == 0)


def test_sweep_grid_is_exact_in_both_matmul_modes():
    """12 significant bits: s_j * x is exact in f32, and x = bf16 hi + bf16 lo exactly (what makes the bf16x3 projection exact as well)"""
    g = R.sweep_grid()
    assert g.size == 2 + 2 * len(R.SWEEP_MAGNITUDES) and np.signbit(g[1]) and g[1] == 0
    bits = g.view(np.uint32)
    assert np.all(bits & 0x7FF == 0)              # 23 - 11 mantissa bits used
    hi = (bits & 0xFFFF0000).view(f32)
    lo = (g - hi).astype(f32)
    assert np.all((lo.view(np.uint32) & 0xFFFF) == 0) and np.array_equal((hi.astype(np.float64) + lo), g.astype(np.float64))
    fin = np.abs(g) < 1e38
    for s in R.sweep_scales(9):
        assert np.array_equal((g[fin] * f32(s)).astype(np.float64), g[fin].astype(np.float64) * s)


@pytest.mark.parametrize("cell", ["lstm", "gru", "tanh"])
@pytest.mark.parametrize("whh", [0.0, 0.5])
def test_sweep_bounds_restate_the_reference(cell, whh):
    """The bound propagation walks the same equations as the reference (which torch checks above): same values.  With W_hh = 0 the
    pre-activations are exact, so the bound of a saved activation is the 3e-7 claim itself; nowhere is a bound so wide that it says nothing."""
    case = R.sweep_case(cell, 32, whh)
    ref = R.run(cell, case)
    for prec in (0, 1):
        b = R.sweep_bounds(cell, case, prec)
        for k in ("act", "aux", "y", "da", "daux", "dx"):
            if cell == "tanh" and k in ("aux", "daux"):
                continue
            assert b[k].v.shape == ref[k].shape, k
            assert R.max_abs(b[k].v, ref[k]) <= 1e-12 * max(1.0, float(np.max(np.abs(ref[k])))), k
            assert np.all(np.isfinite(b[k].e)) and np.all(b[k].e >= 0), k
        if whh == 0.0:
            assert np.all(b["act"].e == R.ACT_EPS)
        # (precision 1 with a live W_hh: the split's 2^-16 of a recurrent sum of up to 0.5 is 7.6e-6 by itself)
        wide = 10.0 if (prec == 1 and whh != 0.0) else 1.0
        assert np.max(b["act"].e) < 2e-6 * wide and np.median(b["y"].e) < 2e-6 and np.max(b["y"].e) < 5e-6 * wide
        assert np.max(b["da"].e) < 1e-5 * wide * max(1.0, float(np.max(np.abs(ref["da"]))))
        assert np.max(b["dx"].e) < 1e-4 * wide * max(1.0, float(np.max(np.abs(ref["dx"]))))
