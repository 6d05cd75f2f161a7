"""The BatchNorm entry points of norm.hip against float64, outside the Gaussian regime.

Everywhere else in the suite BatchNorm sees a * N(0,1) + b with a in 1.7-3, |b| <= 1.5 under an absolute gate of 2e-5.  There the
ss / n - mean^2 form of the variance, its clamp at 0, (x - fl32(mean)) * rstd with a mean that is large against the spread, rstd =
1 / sqrt(eps) on a dead channel, g - s0 / n under a common component of dy and the count guards are all idle.  Here every channel of a test
tensor is one REGIME of tests/bn_ref.py (log-mel features at 15 +- 3, offsets of 1e3 / 1e5 / 300 +- 0.03, constants, 98 % zeros, one spike,
var << eps, std 1e6 and 1e15, two values one ulp apart) crossed with a regime of dy (N(0,1), 1 + 1e-3 N, 1e-6 N, zero), and every output is
held to the float64 restatement within a per-element / per-channel bound DERIVED from the kernel's stated arithmetic (bn_ref.bounds; the
derivation is in its docstring, tests/test_bn_regimes_host.py shows that the stated arithmetic meets the bounds and that they are not
vacuous).  On the control channels (gauss x under gauss dy) the suite's rel-L2 1e-5 gate on dgamma / dbeta is kept next to the bound.

Shapes (outer, C, inner), the smallest that reach each launch branch (test_batchnorm_branch_matrix_vs_oracle and
test_full_length_masked_kernels_equal_dense_bit_for_bit establish them):
  rows   27 x 14             C % 4 != 0: dword column sums, V = 1 apply / dx
  rows   200 x 28            rows4 sums, bn_apply_rows4_kernel / bn_dx_rows4_kernel
  rows   1500 x 84, x at storage offset 1    the dword kernels although C % 4 == 0; several row chunks
  rows   400 x 84, option bn_rows4 = 0       a ragged second 64-column block; held bit for bit to bn_rows4 = 1
  NCHW   3 x 14 x 200        16-B loads;   2 x 14 x 33   scalar loads;   3 x 14 x 28000   planes cut (ich > 1);   200 x 28 x 37   opc > 1
Through the C ABI, outputs and workspace NaN-filled: ctcn_bn_fwd_train (ReLU off / on), ctcn_bn_bwd (beta_acc 0 / 1), ctcn_bn_fwd_eval from
the kernel's own running statistics and from a grid of running_var in {0, 1e-12, 1e-5, 1, 1e8} x running_mean in {0, +-15, +-1e5}; the
length-aware entry points with x and dy NaN at every invalid element, incl. n = 1 and n = 0; the dropout-fused pair and the synchronised
pair bit for bit / within the bounds.  With ReLU the kernel's mask must be the oracle's wherever |y_ref| exceeds its bound, and the backward
reference takes the kernel's own mask.  Constant channels must come out exact.  A second call gives the same bits.  And bn_value /
bn_dx_value are held as a BIT contract: replayed in numpy from the kernel's own save_mean, save_rstd, dbeta and dgamma they give the kernel's
y and dx (an equally accurate reordering, e.g. fma(x - m, rs * g, b), stays inside every error bound and was seen to pass everything else).

CTCN_REGIME_LOG=<file>: one JSON line per case with max(error / bound) per output (the record the figures in the commit message come from).
"""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as B  # noqa: E402

gpu = pytest.mark.gpu
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ctcn.h")
DENSE = [c for c in B.CASES if c != B.SYNC_CASE]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _log(record):
    path = os.environ.get("CTCN_REGIME_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class _rows4(object):
    """option bn_rows4 for the duration of a `with`, then what was there before"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from ctc_pytorch_amd import _lib
        self.before = _lib.lib().ctcn_get_option(b"bn_rows4")
        _lib.check(_lib.lib().ctcn_set_option(b"bn_rows4", self.value), "set_option")

    def __exit__(self, *exc):
        from ctc_pytorch_amd import _lib
        _lib.lib().ctcn_set_option(b"bn_rows4", self.before)


class Device(object):
    """A bn_ref case on the device: x at its storage offset, x / dy NaN at every invalid element, and the calls."""

    def __init__(self, dev, case, masked=None):
        from ctc_pytorch_amd import _lib
        self.L, self.lib, self.dev = _lib.lib(), _lib, dev
        self.t = t = B.make_case(case, masked)
        self.layout, self.shape, xoff, self.rows4 = B.CASES[case]
        self.outer, self.C, self.inner = self.shape
        self.valid = t.get("valid")
        poison = (lambda a: np.array(a)) if self.valid is None else (lambda a: np.where(self.valid, a, np.float32("nan")).astype(np.float32))
        buf = torch.zeros(t["x"].size + xoff, device=dev)
        self.x = buf[xoff:].view(self.shape)
        self.x.copy_(torch.from_numpy(poison(t["x"])))
        assert self.x.data_ptr() % 16 == 4 * xoff
        self.dy = torch.from_numpy(poison(t["dy"])).to(dev)
        up = lambda k: torch.from_numpy(np.array(t[k])).to(dev)
        self.gamma, self.beta, self.rm0, self.rv0 = up("gamma"), up("beta"), up("rm0"), up("rv0")
        self.geom = ()
        if masked is not None:
            _, lens, batch, frame = B.MASKED_CASES[masked]
            self.lens = torch.tensor(lens, dtype=torch.int32, device=dev)
            self.geom = (P(self.lens), batch, frame)
        need = (self.L.ctcn_bn_masked_ws_bytes if self.geom else self.L.ctcn_bn_ws_bytes)(*self.shape)
        assert need > 0
        self.ws = torch.full((int(need) // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
        self.st = _lib.stream_ptr()

    def nan(self, *shape):
        return torch.full(shape or self.shape, float("nan"), device=self.dev)

    def wsb(self):
        self.ws.fill_(float("nan"))
        return P(self.ws), self.ws.numel() * 8

    def forward(self, relu):
        o = {"y": self.nan(), "save_mean": self.nan(self.C), "save_rstd": self.nan(self.C), "running_mean": self.rm0.clone(),
             "running_var": self.rv0.clone(), "nbt": torch.zeros((), dtype=torch.int64, device=self.dev)}
        a = (P(self.x), P(o["y"]), P(self.gamma), P(self.beta), P(o["running_mean"]), P(o["running_var"]), P(o["save_mean"]), P(o["save_rstd"]))
        b = self.shape + (B.EPS, B.MOM, int(relu)) + self.wsb() + (self.st, P(o["nbt"]))
        if self.geom:
            self.lib.check(self.L.ctcn_bn_fwd_train_masked(*(a + self.geom + b)), "fwd_train_masked")
        else:
            self.lib.check(self.L.ctcn_bn_fwd_train(*(a + b)), "fwd_train")
        return o

    def backward(self, f, relu, acc, dy=None):
        t = self.t
        o = {"dx": self.nan(), "dgamma": torch.from_numpy(t["base_g"].copy()).to(self.dev) if acc else self.nan(self.C),
             "dbeta": torch.from_numpy(t["base_b"].copy()).to(self.dev) if acc else self.nan(self.C)}
        a = (P(self.x), P(f["y"]) if relu else None, P(self.dy if dy is None else dy), P(self.gamma), P(f["save_mean"]), P(f["save_rstd"]), P(o["dx"]),
             P(o["dgamma"]), P(o["dbeta"]))
        b = self.shape + (int(relu), 1.0 if acc else 0.0) + self.wsb() + (self.st,)
        if self.geom:
            self.lib.check(self.L.ctcn_bn_bwd_masked(*(a + self.geom + b)), "bwd_masked")
        else:
            self.lib.check(self.L.ctcn_bn_bwd(*(a + b)), "bwd")
        return o

    def evaluate(self, rm, rv, relu):
        y = self.nan()
        a = (P(self.x), P(y), P(self.gamma), P(self.beta), P(rm), P(rv))
        b = self.shape + (B.EPS, int(relu), self.st)
        if self.geom:
            self.lib.check(self.L.ctcn_bn_fwd_eval_masked(*(a + self.geom + b)), "fwd_eval_masked")
        else:
            self.lib.check(self.L.ctcn_bn_fwd_eval(*(a + b)), "fwd_eval")
        return y


def _within(got, ref, bnd, what, valid=None):
    """assert |got - ref| <= bnd everywhere (invalid elements: exactly 0); returns max(error / bound)"""
    g = _np(got)
    assert np.isfinite(g).all(), what
    if valid is not None and g.ndim == 3:
        assert np.all(g[~valid] == 0), what
    err = np.abs(g - ref)
    q = B.ratio(err, bnd)
    assert np.all(err <= bnd), (what, q, int(np.argmax(np.where(err == 0, 0, err / np.maximum(bnd, 1e-300)))))
    return q


def _run_case(dev, case, masked, relu):
    d = Device(dev, case, masked)
    t, v = d.t, d.valid
    allv = np.ones(d.shape, dtype=bool) if v is None else v
    rec = {"test": "bn", "case": masked or case, "relu": int(relu)}
    with _rows4(d.rows4):
        f = d.forward(relu)
        ref, bnd, fwd = B.reference(t, relu)
        assert int(f["nbt"]) == 1
        for k in ("save_mean", "save_rstd", "running_mean", "running_var", "y"):
            rec[k] = _within(f[k], ref[k], bnd[k], (case, masked, relu, k), v)
        # bn_value is a bit contract: replayed from the kernel's own save_mean / save_rstd it gives the kernel's y
        xz = np.where(allv, t["x"].astype(np.float64), 0.0)
        m32, rs32 = _np(f["save_mean"]), _np(f["save_rstd"])
        want = B.model_value(xz, B._b(m32), B._b(rs32), B._b(t["gamma"].astype(np.float64)), B._b(t["beta"].astype(np.float64)))
        want = np.where(allv, np.maximum(want, 0.0) if relu else want, 0.0)
        rec["y replay mismatch"] = float(np.mean(_np(f["y"]) != want))
        assert rec["y replay mismatch"] <= B.REPLAY_MISMATCH, rec
        mask = None
        if relu:
            mask = (_np(f["y"]) > 0) & allv
            sure = allv & (np.abs(fwd["y"]) > bnd["y"])
            assert np.array_equal(mask[sure], fwd["y"][sure] > 0)
        outs = [f]
        ctl = B.control_channels(case) if masked is None else []
        for acc in (False, True):
            ref, bnd, fwd = B.reference(t, relu, mask, acc)          # the backward reference takes the kernel's own mask
            b = d.backward(f, relu, acc)
            for k in ("dx", "dgamma", "dbeta"):
                rec["%s acc%d" % (k, acc)] = _within(b[k], ref[k], bnd[k], (case, masked, relu, acc, k), v)
            outs.append(b)
            if not acc:                                              # bn_dx_value likewise, from the sums the kernel stored as dbeta / dgamma
                g = np.where(allv if mask is None else mask, t["dy"].astype(np.float64), 0.0)
                want = B.model_dx(xz, g, t["gamma"].astype(np.float64), m32, rs32, _np(b["dbeta"]), _np(b["dgamma"]), fwd["n"], allv)
                rec["dx replay mismatch"] = float(np.mean(_np(b["dx"]) != want))
                assert rec["dx replay mismatch"] <= B.REPLAY_MISMATCH, rec
            if ctl and not acc:                                      # the Gaussian regime keeps the suite's gate next to the bound
                for k in ("dgamma", "dbeta"):
                    rec["control rel-L2 " + k] = B.rel_l2(_np(b[k])[ctl], ref[k][ctl])
                    assert rec["control rel-L2 " + k] <= B.CONTROL_REL_L2, (k, rec)
        # constant channels (and every channel of the n = 1 cases) are exact
        sm, sr, rv, y = _np(f["save_mean"]), f["save_rstd"].cpu().numpy(), f["running_var"].cpu().numpy(), f["y"].cpu().numpy()
        rs0 = np.float32(1.0 / np.sqrt(B.EPS))
        for c in np.flatnonzero(B._const_exact(xz, allv, fwd["n"])):
            a = xz[:, c, :][allv[:, c, :]][0]
            want = np.float32(max(t["beta"][c], 0.0) if relu else t["beta"][c])
            assert sm[c] == a and np.all(y[:, c, :][allv[:, c, :]] == want), (c, t["regimes"][c])
            assert abs(float(sr[c]) - float(rs0)) <= float(np.spacing(rs0)), (c, sr[c])
            assert rv[c] == np.float32((1.0 - B.MOM) * float(t["rv0"][c])), (c, rv[c])
        if fwd["n"] == 0:
            assert not sm.any() and np.all(np.abs(sr - rs0) <= np.spacing(rs0)) and not _np(b["dx"]).any()
        # the eval forward, from the kernel's own running statistics and from the eval-only grid
        grid = (torch.from_numpy(t["eval_rm"].copy()).to(dev), torch.from_numpy(t["eval_rv"].copy()).to(dev))
        for tag, (rm, rvv) in (("own", (f["running_mean"], f["running_var"])), ("grid", grid)):
            ye = d.evaluate(rm, rvv, relu)
            args = (t["x"], t["gamma"], t["beta"], _np(rm), _np(rvv), v)
            rec["eval " + tag] = _within(ye, B.eval_fwd(*args, relu=relu), B.eval_bounds(*args), (case, masked, relu, "eval", tag), v)
            outs.append({"eval": ye})
        # the same input bits give the same output bits
        f2 = d.forward(relu)
        again = [f2, d.backward(f2, relu, False), d.backward(f2, relu, True), {"eval": d.evaluate(f2["running_mean"], f2["running_var"], relu)},
                 {"eval": d.evaluate(grid[0], grid[1], relu)}]
        for o1, o2 in zip(outs, again):
            for k in o1:
                assert torch.equal(o1[k], o2[k]), (case, masked, k)
    if d.rows4 == 0:                                                 # the dword reductions by option: every output equals the default's bits
        d1 = Device(dev, case, masked)
        f1 = d1.forward(relu)
        for o1, o2 in ((f, f1), (outs[1], d1.backward(f1, relu, False))):
            for k in o1:
                assert torch.equal(o1[k], o2[k]), (case, "bn_rows4", k)
    torch.cuda.synchronize()
    _log(rec)
    return rec


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", DENSE)
def test_dense_entry_points_within_bounds(dev, case, relu):
    """ctcn_bn_fwd_train / ctcn_bn_bwd / ctcn_bn_fwd_eval on every launch branch, every regime in every tensor."""
    _run_case(dev, case, None, relu)


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("masked", list(B.MASKED_CASES))
def test_length_aware_entry_points_within_bounds(dev, masked, relu):
    """ctcn_bn_fwd_train_masked / ctcn_bn_bwd_masked / ctcn_bn_fwd_eval_masked: the same bounds over the valid elements, x and dy NaN at
    every invalid one, lens with a full-length, a one-frame and a zero-length utterance.  The `_n1` cases leave one valid element per
    channel (mean = the value, var 0, running_var updated with the biased value: count > 1 guards the n / (n - 1)), the `_n0` cases none
    (mean 0, var 0, y = dx = 0, dgamma / dbeta 0 or their beta_acc base: count > 0 guards s / n) -- bn_finalize_stats_kernel's two rules."""
    rec = _run_case(dev, B.MASKED_CASES[masked][0], masked, relu)
    assert all(np.isfinite(q) for k, q in rec.items() if isinstance(q, float))


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case,batch,frame", [("rows_200x28", 4, 1), ("nchw_3x14x200", 3, 8)])
def test_full_lengths_equal_dense_bit_for_bit_on_regime_data(dev, case, batch, frame, relu):
    """The property of test_full_length_masked_kernels_equal_dense_bit_for_bit where the sums cancel and the means are large."""
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    d = Device(dev, case)
    outer, C, inner = d.shape
    tmax = outer // batch if d.layout == "rows" else inner // frame
    lens = torch.tensor([tmax] * batch, dtype=torch.int32, device=dev)
    ws = torch.full((int(L.ctcn_bn_masked_ws_bytes(outer, C, inner)) // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
    f = d.forward(relu)
    b = d.backward(f, relu, False)
    ye = d.evaluate(d.rm0, d.rv0, relu)
    m = {"y": d.nan(), "save_mean": d.nan(C), "save_rstd": d.nan(C), "running_mean": d.rm0.clone(), "running_var": d.rv0.clone(), "dx": d.nan(),
         "dgamma": d.nan(C), "dbeta": d.nan(C), "eval": d.nan()}
    _lib.check(L.ctcn_bn_fwd_train_masked(P(d.x), P(m["y"]), P(d.gamma), P(d.beta), P(m["running_mean"]), P(m["running_var"]), P(m["save_mean"]),
                                          P(m["save_rstd"]), P(lens), batch, frame, outer, C, inner, B.EPS, B.MOM, int(relu), P(ws), ws.numel() * 8, d.st,
                                          None), "fwd_train_masked")
    _lib.check(L.ctcn_bn_bwd_masked(P(d.x), P(m["y"]) if relu else None, P(d.dy), P(d.gamma), P(m["save_mean"]), P(m["save_rstd"]), P(m["dx"]),
                                    P(m["dgamma"]), P(m["dbeta"]), P(lens), batch, frame, outer, C, inner, int(relu), 0.0, P(ws), ws.numel() * 8, d.st),
               "bwd_masked")
    _lib.check(L.ctcn_bn_fwd_eval_masked(P(d.x), P(m["eval"]), P(d.gamma), P(d.beta), P(d.rm0), P(d.rv0), P(lens), batch, frame, outer, C, inner, B.EPS,
                                         int(relu), d.st), "fwd_eval_masked")
    torch.cuda.synchronize()
    dense = dict(f, eval=ye, **b)
    for k in m:
        assert bool(torch.isfinite(dense[k]).all()), k
        assert torch.equal(m[k], dense[k]), (k, float((m[k] - dense[k]).abs().max()))


@gpu
@pytest.mark.parametrize("case", B.DROPOUT_CASES)
def test_dropout_fused_pair_equals_two_passes_on_regime_data(dev, case):
    """ctcn_bn_fwd_train_dropout == ctcn_bn_fwd_train then ctcn_dropout, ctcn_bn_bwd_dropout == ctcn_dropout on the gradient then ctcn_bn_bwd,
    bit for bit, ReLU on, p = 0.3: the backward pass recomputes the ReLU mask from x, and the offset regimes put many y next to 0, where
    one different rounding would flip it
    (test_bn_regimes_host.py: such elements exist in both cases)."""
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    d = Device(dev, case)
    outer, C, inner = d.shape
    n = d.x.numel()
    p, seed, off = 0.3, 1234, 77
    f = d.forward(True)
    yd = d.nan()
    _lib.check(L.ctcn_dropout(P(f["y"]), P(yd), n, p, seed, off, d.st), "dropout")
    fu = {"y": d.nan(), "save_mean": d.nan(C), "save_rstd": d.nan(C), "running_mean": d.rm0.clone(), "running_var": d.rv0.clone()}
    wp, wn = d.wsb()
    _lib.check(L.ctcn_bn_fwd_train_dropout(P(d.x), P(fu["y"]), P(d.gamma), P(d.beta), P(fu["running_mean"]), P(fu["running_var"]), P(fu["save_mean"]),
                                           P(fu["save_rstd"]), outer, C, inner, B.EPS, B.MOM, 1, wp, wn, d.st, None, p, seed, off), "fwd_train_dropout")
    assert torch.equal(fu["y"], yd) and bool(torch.isfinite(yd).all())
    for k in ("save_mean", "save_rstd", "running_mean", "running_var"):
        assert torch.equal(fu[k], f[k]), k
    g = d.nan()
    _lib.check(L.ctcn_dropout(P(d.dy), P(g), n, p, seed, off, d.st), "dropout of dy")
    two = d.backward(f, True, False, dy=g)
    fb = {"dx": d.nan(), "dgamma": d.nan(C), "dbeta": d.nan(C)}
    wp, wn = d.wsb()
    _lib.check(L.ctcn_bn_bwd_dropout(P(d.x), P(d.dy), P(d.gamma), P(d.beta), P(f["save_mean"]), P(f["save_rstd"]), P(fb["dx"]), P(fb["dgamma"]),
                                     P(fb["dbeta"]), outer, C, inner, 1, 0.0, wp, wn, d.st, p, seed, off), "bwd_dropout")
    torch.cuda.synchronize()
    for k in fb:
        assert bool(torch.isfinite(fb[k]).all()) and torch.equal(fb[k], two[k]), (k, float((fb[k] - two[k]).abs().max()))


@gpu
@pytest.mark.parametrize("relu", [False, True])
def test_synchronised_pair_on_unequal_shards(dev, relu):
    """ctcn_bn_fwd_sums / _fwd_finish / ctcn_bn_bwd_sums / _bwd_finish on two shards of 130 and 270 rows whose gauss and logmel channels sit at
    -50 and +50: the global variance is mostly between the shards.  Adding the shards' float64 sums is a summation order like any other, so
    the results are held to the bounds of the full-batch reference; and they equal the single-call dense results within the 2e-6 of
    test_sync_batchnorm_two_shards_equal_full_batch (of max(1, |value|): 2e-6 is below the float32 spacing of the larger values here)."""
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    d = Device(dev, B.SYNC_CASE)
    t, (rows, C, inner) = d.t, d.shape
    cuts = [(0, B.SYNC_SHARDS[0]), (B.SYNC_SHARDS[0], rows)]
    parts = [(d.x[a:b].contiguous(), d.dy[a:b].contiguous()) for a, b in cuts]
    total = float(rows * inner)
    f, sums = d.forward(relu), []
    for xs, _ in parts:
        sm = torch.full((C, 2), float("nan"), dtype=torch.float64, device=dev)
        wp, wn = d.wsb()
        _lib.check(L.ctcn_bn_fwd_sums(P(xs), P(sm), xs.shape[0], C, inner, wp, wn, d.st), "fwd_sums")
        sums.append(sm)
    glob = sums[0] + sums[1]
    fs = []
    for xs, _ in parts:
        o = {"y": torch.full_like(xs, float("nan")), "save_mean": d.nan(C), "save_rstd": d.nan(C), "running_mean": d.rm0.clone(), "running_var": d.rv0.clone()}
        _lib.check(L.ctcn_bn_fwd_finish(P(xs), P(o["y"]), P(d.gamma), P(d.beta), P(o["running_mean"]), P(o["running_var"]), P(o["save_mean"]),
                                        P(o["save_rstd"]), P(glob), total, xs.shape[0], C, inner, B.EPS, B.MOM, int(relu), d.st, None), "fwd_finish")
        fs.append(o)
    ref, bnd, fwd = B.reference(t, relu)
    rec = {"test": "bn_sync", "relu": int(relu)}
    y = torch.cat([o["y"] for o in fs])
    rec["y"] = _within(y, ref["y"], bnd["y"], "sync y")
    for o in fs:
        for k in ("save_mean", "save_rstd", "running_mean", "running_var"):
            rec[k] = _within(o[k], ref[k], bnd[k], "sync " + k)
            assert torch.equal(o[k], fs[0][k]), k
    close = lambda a, b: bool(((a - b).abs() <= 2e-6 * b.abs().clamp(min=1.0)).all())
    assert close(y, f["y"]) and all(close(fs[0][k], f[k]) for k in ("save_mean", "save_rstd", "running_mean", "running_var"))
    mask = (_np(y) > 0) if relu else None
    ref, bnd, fwd = B.reference(t, relu, mask)
    lsum = []
    for (xs, ds), o in zip(parts, fs):
        sm = torch.full((C, 2), float("nan"), dtype=torch.float64, device=dev)
        wp, wn = d.wsb()
        _lib.check(L.ctcn_bn_bwd_sums(P(xs), P(o["y"]), P(ds), P(o["save_mean"]), P(o["save_rstd"]), P(sm), xs.shape[0], C, inner, int(relu), wp, wn, d.st),
                   "bwd_sums")
        lsum.append(sm)
    gsum = lsum[0] + lsum[1]
    bs = []
    for (xs, ds), o, sm in zip(parts, fs, lsum):
        b = {"dx": torch.full_like(xs, float("nan")), "dgamma": d.nan(C), "dbeta": d.nan(C)}
        wp, wn = d.wsb()
        _lib.check(L.ctcn_bn_bwd_finish(P(xs), P(o["y"]), P(ds), P(d.gamma), P(o["save_mean"]), P(o["save_rstd"]), P(b["dx"]), P(b["dgamma"]), P(b["dbeta"]),
                                        P(sm), P(gsum), total, xs.shape[0], C, inner, int(relu), 0.0, wp, wn, d.st), "bwd_finish")
        bs.append(b)
    dx = torch.cat([b["dx"] for b in bs])
    rec["dx"] = _within(dx, ref["dx"], bnd["dx"], "sync dx")
    for k in ("dgamma", "dbeta"):                            # each shard's share is rounded to float32 on its own: u |share| each on top of the bound
        a0, a1 = _np(bs[0][k]), _np(bs[1][k])
        rec[k] = _within(bs[0][k].double() + bs[1][k].double(), ref[k], bnd[k] + 2 * B.U * (np.abs(a0) + np.abs(a1)), "sync " + k)
    dense = d.backward(f, relu, False)
    assert close(dx, dense["dx"])
    for k in ("dgamma", "dbeta"):                            # (rel-L2 1e-6, as there)
        assert B.rel_l2(_np(bs[0][k]) + _np(bs[1][k]), _np(dense[k])) < 1e-6, k
    torch.cuda.synchronize()
    _log(rec)


def test_every_bn_entry_point_is_called_here():
    """The ctcn_bn_* names of include/ctcn.h are the ones this file calls: a later entry point cannot go untested silently."""
    declared = set(re.findall(r"\b(ctcn_bn_\w+)\s*\(", open(HEADER).read()))
    called = set(re.findall(r"\bL\.(ctcn_bn_\w+)", open(os.path.abspath(__file__).replace(".pyc", ".py")).read()))
    assert len(declared) >= 14 and called == declared, sorted(called ^ declared)
