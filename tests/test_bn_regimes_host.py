"""The float64 restatement of BatchNorm, its regimes and its derived bounds, checked without a GPU (no gpu marker).

tests/test_bn_regimes.py holds the thirteen BatchNorm entry points of norm.hip to tests/bn_ref.py outside the Gaussian regime.  That only
means something if (1) the restatement is right, (2) every regime is what its name says at every shape the GPU test uses, (3) the bounds
are satisfiable by the kernel's stated arithmetic at all -- `bn_ref.kernel_model` stays inside them on every tensor the GPU test runs --
and (4) no bound is so wide that it proves nothing.  Those are checked here.

(1) is held to torch.nn.BatchNorm1d / BatchNorm2d in float64 at 1e-12 RELATIVE TO THE TERMS an output is formed from, not to the output:
two float64 evaluations of y = beta + gamma rstd x - gamma rstd mean differ by a few 2^-53 of those terms, which for `const_neg`
(4.7e2 * 3e4 against |y| < 1) is 1e-9 of y.  The scales: y: |beta| + |gamma| rstd (max|x| + |mean|);  dx: |gamma| rstd (max|dy| + sum|dy| / n +
max|xhat| rstd sum|dy| (|x| + |mean|) / n);  dgamma: rstd sum|dy| (|x| + |mean|);  dbeta: sum|dy|;  running mean / var: |rm0| + |mean|,
|rv0| + mean(x^2).  Measured against the outputs themselves the two agree to 1e-12 everywhere but on const_neg (y 1e-9), twopoint (y 2e-10,
dgamma 6e-11) and spike (dx 5e-6: the spike's own element, where 1 - 1/n - xhat^2 / n cancels to 1e-10 of its terms).

(3), measured: the largest model error / bound over all cases, per output --
  save_mean 1.00  save_rstd 0.96  running_mean 0.96  running_var 0.90  y 0.97  dx 0.84  dgamma 0.92  dbeta 0.95  eval y 0.98
(near 1 wherever one float32 rounding is all there is: u |value| is both the bound and, at worst, the error).
torch's own float32 module on the same data (logged, no gate) does NOT stay inside: its sums are float32.  Largest error / bound: dgamma 2.5,
running_var 21, dx 33, dbeta 230, running_mean 725, and y 1e7 on the constant channels, where the bound is that of exact statistics
(torch's float32 mean of n copies of -3e4 is not -3e4).  On the MI355X the kernel's ratios equal the model's to three digits, and its y and dx
equal the model's replay bit for bit.

(4), the caps (conditions, asserted; u = 2^-24):
  * every regime but twopoint, const*, offset_tight: bound(y) <= 1e-2 max|y| of its channel (measured: <= 3e-4; offset_tight itself 1.4e-3)
  * gauss: bound(y), bound(dx) <= 2e-5, the gates of test_batchnorm_branch_matrix_vs_oracle.  Its rel-L2 1e-5 on dgamma / dbeta cannot be
    met by a worst-case bound at every n: the bound of a sum of n roundings grows as n (2 u n E|dy xhat|) against sqrt(n) of the sum itself,
    2.3e-5 of dgamma at n = 7 400.  So on the control channels (gauss x under gauss dy; bn_ref.control_channels) the present gate is KEPT
    NEXT TO the bound -- rel-L2 <= 1e-5 over those channels, asserted here of the model and in the GPU test of the kernel -- and the
    gate in force there is the tighter of the two.
  * offset_tight: bound(y) ~ |gamma| rstd ulp(300) / 2 = 1.5 * 33 * 1.5e-5 = 7e-4 of |y| ~ 1: save_mean is a float32, and the element x - m is
    exact, so the whole error of m reaches y.  Nothing tighter can be asked without a wider save_mean.
  * twopoint: bound(y) = 0.1-0.24 for |y - beta| <= 0.12: fl32(mean) is one of the two values, xhat (+-0.08) is off by as much as it is
    large, and e_var = 3 n 2^-53 4096^2 = 5.6e-9 n passes eps = 1e-5 at n = 1 800.  The bound there says: finite, of the right order, and
    on the right side of the ReLU (|beta| >= 0.5).
  With ReLU, elements with |y_ref| <= bound(y) may fall either side: their share is at most 1 % in every case (measured: <= 5e-4).

CTCN_REGIME_LOG=<file>: one JSON line per case with the model's and torch float32's distances (the latter for comparison only, no gate).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402

# every tensor the GPU test runs: (case, masked-case name or None)
TENSORS = [(name, None) for name in B.CASES] + [(B.MASKED_CASES[m][0], m) for m in B.MASKED_CASES]
IDS = [m or c for c, m in TENSORS]
# torch's BatchNorm is not defined on fewer than two values per channel
TORCH_TENSORS = [(c, m) for c, m in TENSORS if m is None or sum(B.MASKED_CASES[m][1]) * B.MASKED_CASES[m][3] >= 2]
WIDE = ("twopoint", "const0", "const", "const_neg", "offset_tight")


def _log(record):
    path = os.environ.get("CTCN_REGIME_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def _rows(a, sel):
    """(outer, C, inner) -> (n, C) of the valid positions"""
    return np.asarray(a).transpose(0, 2, 1)[sel]


def _torch_bn(t, dtype, relu, two_d=False):
    """torch.nn.BatchNorm1d on the (n, C) matrix of the valid elements (BatchNorm2d on the dense NCHW tensor), training step + eval:
    {y, dx, dgamma, dbeta, running_mean, running_var, eval_y} as float64 numpy in that layout"""
    C = t["x"].shape[1]
    v = t.get("valid", np.ones(t["x"].shape, dtype=bool))
    sel = v[:, 0, :]
    pick = (lambda a: np.asarray(a)[:, :, None, :]) if two_d else (lambda a: _rows(a, sel))
    m = (torch.nn.BatchNorm2d if two_d else torch.nn.BatchNorm1d)(C, eps=B.EPS, momentum=B.MOM).to(dtype)
    with torch.no_grad():
        for p, k in ((m.weight, "gamma"), (m.bias, "beta"), (m.running_mean, "rm0"), (m.running_var, "rv0")):
            p.copy_(torch.tensor(t[k], dtype=dtype))
    x = torch.tensor(pick(t["x"]), dtype=dtype, requires_grad=True)
    y = m(x)
    y = torch.relu(y) if relu else y
    y.backward(torch.tensor(pick(t["dy"]), dtype=dtype))
    m.eval()
    with torch.no_grad():
        ye = m(x)
        ye = torch.relu(ye) if relu else ye
    n64 = lambda a: a.detach().double().numpy().copy()
    back = (lambda a: a[:, :, 0, :]) if two_d else (lambda a: a)
    return {"y": back(n64(y)), "dx": back(n64(x.grad)), "dgamma": n64(m.weight.grad), "dbeta": n64(m.bias.grad),
            "running_mean": n64(m.running_mean), "running_var": n64(m.running_var), "eval_y": back(n64(ye))}, sel


def _scales(t, ref, fwd, bwd_g, sel, two_d):
    """the magnitudes of the terms each output is formed from (module docstring), per channel"""
    v = t.get("valid", np.ones(t["x"].shape, dtype=bool))
    n = fwd["n"]
    ax = np.where(v, np.abs(t["x"].astype(np.float64)), 0.0)
    g = np.abs(bwd_g)
    ga, rstd, mean = np.abs(t["gamma"].astype(np.float64)), fwd["rstd"], np.abs(fwd["mean"])
    cond = rstd * (g * (ax + B._b(mean))).sum(axis=(0, 2))
    return {"y": np.abs(t["beta"]) + ga * rstd * (ax.max(axis=(0, 2)) + mean),
            "dx": ga * rstd * (g.max(axis=(0, 2)) + g.sum(axis=(0, 2)) / n + np.abs(fwd["xhat"]).max(axis=(0, 2)) * cond / n),
            "dgamma": cond, "dbeta": g.sum(axis=(0, 2)), "running_mean": np.abs(t["rm0"]) + mean,
            "running_var": np.abs(t["rv0"]) + (ax * ax).sum(axis=(0, 2)) / n}


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case,masked", TORCH_TENSORS, ids=[m or c for c, m in TORCH_TENSORS])
def test_restatement_agrees_with_torch_float64(case, masked, relu):
    t = B.make_case(case, masked)
    ref, _, fwd = B.reference(t, relu)
    two_d = masked is None and B.CASES[case][0] == "nchw"
    got, sel = _torch_bn(t, torch.float64, relu, two_d)
    keep = (fwd["y"] > 0) if relu else np.ones(t["x"].shape, dtype=bool)
    scale = _scales(t, ref, fwd, np.where(keep & t.get("valid", True), t["dy"].astype(np.float64), 0.0), sel, two_d)
    lay = (lambda a: a) if two_d else (lambda a: _rows(a, sel))
    for k in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        d = np.abs(got[k] - lay(ref[k]) if ref[k].ndim == 3 else got[k] - ref[k])
        d = d.max(axis=(0, 2) if two_d else 0) if d.ndim > 1 else d
        assert np.all(d <= 1e-12 * scale[k]), (k, [(t["regimes"][c], d[c], scale[k][c]) for c in np.flatnonzero(d > 1e-12 * scale[k])])
    # eval: from the running statistics torch has just produced
    ye = B.eval_fwd(t["x"], t["gamma"], t["beta"], got["running_mean"], got["running_var"], t.get("valid"), relu=relu)
    d = np.abs(got["eval_y"] - lay(ye))
    d = d.max(axis=(0, 2) if two_d else 0)
    ax = np.where(t.get("valid", True), np.abs(t["x"].astype(np.float64)), 0.0).max(axis=(0, 2))
    s = np.abs(t["beta"]) + np.abs(t["gamma"]) / np.sqrt(got["running_var"] + B.EPS) * (ax + np.abs(got["running_mean"]))
    assert np.all(d <= 1e-12 * s), d / s


def test_every_regime_and_statistics_pair_occurs():
    """84 and 28 channels are multiples of the 14 regimes, so every case holds each regime equally often; over the cases every x regime
    meets every dy regime, and every (running_var, running_mean) pair of the eval-only grid is used."""
    crossed, combos = set(), set()
    for case in B.CASES:
        t = B.make_case(case)
        assert set(t["regimes"]) == set(B.REGIMES), case
        crossed.update(zip(t["regimes"], t["dy_regimes"]))
        combos.update(int(c) for c in t["eval_combo"])
    assert crossed == {(a, b) for a in B.REGIMES for b in B.DY_REGIMES}
    assert combos == set(range(len(B.EVAL_VARS) * len(B.EVAL_MEANS)))
    for m, (case, lens, batch, frame) in B.MASKED_CASES.items():
        layout, (outer, C, inner), _, _ = B.CASES[case]
        tmax = outer // batch if layout == "rows" else inner // frame
        if not (m.endswith("_n0") or m.endswith("_n1")):
            others = [l for mm, (cc, l, _, _) in B.MASKED_CASES.items() if cc == case and not mm.endswith(("_n0", "_n1"))]
            seen = set(sum(others, []))
            assert {tmax, 1, 0} <= seen, (m, seen)
        n = B.make_case(case, m)["valid"][:, 0, :].sum()
        assert n == sum(lens) * frame and (not m.endswith("_n0") or n == 0) and (not m.endswith("_n1") or n == 1)


@pytest.mark.parametrize("case,masked", TENSORS, ids=IDS)
def test_regimes_are_what_they_say(case, masked):
    t = B.make_case(case, masked)
    v = t.get("valid", np.ones(t["x"].shape, dtype=bool))
    n = int(v[:, 0, :].sum())
    if n < 2:
        return
    x = t["x"].astype(np.float64)
    for c, regime in enumerate(t["regimes"]):
        a = x[:, c, :][v[:, c, :]]
        mean, std = a.mean(), a.std()
        big = n >= 1000                                      # sample statistics are only asserted where the sample carries them
        tag = (case, masked, c, regime, mean, std)
        if regime == "gauss" and case != B.SYNC_CASE:
            assert not big or (abs(mean - 0.5) < 0.3 and 1.8 < std < 2.2), tag
        elif regime == "logmel" and case != B.SYNC_CASE:
            assert abs(mean - 15) < 3 and (not big or 2.7 < std < 3.3), tag
        elif regime in ("gauss", "logmel"):                  # the synchronised case: two shards 100 apart, variance mostly between them
            lo, hi = a[:B.SYNC_SHARDS[0]], a[B.SYNC_SHARDS[0]:]
            assert hi.mean() - lo.mean() > 95 and std ** 2 > 100 * max(lo.var(), hi.var()), tag
        elif regime == "offset3":
            assert abs(mean) / std > 500, tag
        elif regime == "offset5":
            assert abs(mean) / std > 2000, tag
        elif regime == "offset_tight":
            assert abs(mean) / std > 5000 and std < 0.06, tag
        elif regime in B.CONST_VALUE:
            assert np.all(a == B.CONST_VALUE[regime]), tag
        elif regime == "sparse":
            assert np.mean(a == 0) >= 0.9 and (not big or (0.97 < np.mean(a == 0) < 0.99 and a.max() > 5)), tag
        elif regime == "spike":
            assert np.sum(a != 0) == 1 and a.max() == 1e3, tag
        elif regime == "tiny":
            assert std ** 2 / B.EPS < 1e-6 and std > 0, tag
        elif regime == "huge":
            assert 3e5 < std < 3e6, tag
        elif regime == "vast":
            assert 3e14 < std < 3e15, tag
        elif regime == "twopoint":
            assert set(np.unique(a)) <= {float(B.TWOPOINT[0]), float(B.TWOPOINT[1])} and float(B.TWOPOINT[1]) - float(B.TWOPOINT[0]) == 2.0 ** -11, tag
            assert not big or 0.4 < np.mean(a == a.max()) < 0.6, tag
    for c, regime in enumerate(t["dy_regimes"]):
        g = t["dy"][:, c, :].astype(np.float64)
        if regime == "common":
            assert abs(g.mean() - 1) < 1e-3 and g.std() < 2e-3
        elif regime == "small":
            assert 0 < np.abs(g).max() < 1e-5
        elif regime == "zero":
            assert not g.any()
    assert np.all((np.abs(t["gamma"]) >= 0.5) & (np.abs(t["gamma"]) <= 1.5)) and (t["gamma"] < 0).any() and (t["gamma"] > 0).any()
    assert np.all(np.abs(t["beta"]) >= 0.05)


def _model_ratios(t, relu, acc):
    """max(error / bound) of kernel_model per output, the bounds, the reference"""
    mod = B.modelled(t, relu, acc)
    ref, bnd, fwd = B.reference(t, relu, (mod["y"] > 0) if relu else None, acc)       # the backward reference takes the model's own mask
    q = {}
    for k in B.OUTPUTS:
        err = np.abs(mod[k] - ref[k])
        assert np.all(err <= bnd[k]), (k, B.ratio(err, bnd[k]))
        q[k] = B.ratio(err, bnd[k])
    return q, mod, ref, bnd, fwd


@pytest.mark.parametrize("case,masked", TENSORS, ids=IDS)
def test_kernel_model_stays_inside_the_bounds(case, masked):
    """What norm.hip states, replayed in float32 / float64, satisfies every gate of the GPU test on every tensor it runs: training forward
    and backward (ReLU off / on, beta_acc 0 / 1), the eval forward from the model's own running statistics and from the eval-only grid."""
    t = B.make_case(case, masked)
    rec = {"test": "bn_host", "case": masked or case}
    for relu in (False, True):
        for acc in (False, True):
            q, mod, ref, bnd, fwd = _model_ratios(t, relu, acc)
            rec["model relu%d acc%d" % (relu, acc)] = q
        for tag, rm, rv in (("own", mod["running_mean"], mod["running_var"]), ("grid", t["eval_rm"], t["eval_rv"])):
            ye = B.model_eval(t["x"], t["gamma"], t["beta"], rm, rv, t.get("valid"), relu)
            want, eb = B.eval_fwd(t["x"], t["gamma"], t["beta"], rm, rv, t.get("valid"), relu=relu), B.eval_bounds(t["x"], t["gamma"], t["beta"], rm, rv, t.get("valid"))
            assert np.all(np.abs(ye - want) <= eb), (tag, B.ratio(np.abs(ye - want), eb))
            rec["model eval %s relu%d" % (tag, relu)] = B.ratio(np.abs(ye - want), eb)
    if fwd["n"] >= 2:                                         # for comparison only: torch's own float32 module on the same data
        two_d = masked is None and B.CASES[case][0] == "nchw"
        got, sel = _torch_bn(t, torch.float32, False, two_d)
        ref, bnd, _ = B.reference(t)
        lay = (lambda a: a) if two_d else (lambda a: _rows(a, sel))
        rec["torch_f32"] = {k: B.ratio(np.abs(got[k] - (lay(ref[k]) if ref[k].ndim == 3 else ref[k])), lay(bnd[k]) if ref[k].ndim == 3 else bnd[k])
                            for k in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")}
    _log(rec)


def test_synchronised_shards_are_the_full_batch():
    """The synchronised pair adds two shards' float64 sums and finishes with the global count: a summation order like any other, so the
    full-batch bounds apply.  Here: the sums of the shards give the statistics of the whole (the restatement, shard by shard)."""
    t = B.make_case(B.SYNC_CASE)
    x = t["x"].astype(np.float64)
    h = B.SYNC_SHARDS[0]
    s = x[:h].sum(axis=(0, 2)) + x[h:].sum(axis=(0, 2))
    fwd = B.train_fwd(t["x"], t["gamma"], t["beta"])
    assert sum(B.SYNC_SHARDS) == x.shape[0] and np.allclose(s / fwd["n"], fwd["mean"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("case", list(B.CASES))
def test_bounds_are_not_vacuous(case):
    t = B.make_case(case)
    for relu in (False, True):
        ref, bnd, fwd = B.reference(t, relu)
        for c, regime in enumerate(t["regimes"]):
            ymax = np.abs(fwd["y"][:, c]).max()             # (before the ReLU, which may leave nothing)
            if regime not in WIDE:
                assert bnd["y"][:, c].max() <= 1e-2 * ymax, (regime, bnd["y"][:, c].max(), ymax)
            if regime == "gauss" and case != B.SYNC_CASE:
                assert bnd["y"][:, c].max() <= 2e-5 and bnd["dx"][:, c].max() <= 2e-5, (bnd["y"][:, c].max(), bnd["dx"][:, c].max())
            if regime in B.CONST_VALUE:                       # the rule for constants: the bounds are those of exact statistics
                assert bnd["save_mean"][c] == 0 and bnd["y"][:, c].max() <= 2 * B.U * np.abs(t["beta"][c])
        ctl = B.control_channels(case)
        if ctl:
            mod = B.modelled(t, relu)
            for k in ("dgamma", "dbeta"):
                assert B.rel_l2(mod[k][ctl], ref[k][ctl]) <= B.CONTROL_REL_L2, (k, relu)


def test_control_channels_exist():
    n = sum(len(B.control_channels(case)) for case in B.CASES)
    assert n >= 3, n


@pytest.mark.parametrize("case,masked", TENSORS, ids=IDS)
def test_relu_edge_share(case, masked):
    """Elements whose sign a float32 kernel may legitimately get either way are at most 1 % of the case."""
    t = B.make_case(case, masked)
    ref, bnd, fwd = B.reference(t, True)
    v = t.get("valid", np.ones(t["x"].shape, dtype=bool))
    unsure = v & (np.abs(fwd["y"]) <= bnd["y"])
    assert unsure.sum() <= 0.01 * max(int(v.sum()), 1), unsure.sum() / max(int(v.sum()), 1)


@pytest.mark.parametrize("case", B.DROPOUT_CASES)
def test_dropout_cases_hold_elements_next_to_the_relu_edge(case):
    """ctcn_bn_bwd_dropout recomputes the ReLU mask from x: the cases it is held on must hold y within 1e-2 of 0 (and some within 1e-3)."""
    t = B.make_case(case)
    y = np.abs(B.train_fwd(t["x"], t["gamma"], t["beta"])["y"])
    assert np.sum(y < 1e-2) >= 5 and np.sum(y < 1e-3) >= 1
