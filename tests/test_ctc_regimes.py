"""The CTC loss kernels of ctc.hip against float64 outside the Gaussian regime: peaked, -inf, barely feasible, un-normalised and uniform
log-probs (tests/ctc_ref.py: the reference, the bounds and their derivation, the regimes; tests/test_ctc_regimes_host.py: what those
rest on).  One batch per launch shape of plan_ctc_lattice, the regimes its utterances; every entry point that reaches the lattice bodies
and the two gradient instantiations; the log-softmax pair on its own inputs; forced alignment where the path is known.

Per form and utterance (ctc_ref.check_utterance): exactly the cells t < in_len, s < 2 L + 1 written; alpha and beta -inf exactly where
the reference is and every finite cell within its bound, bit-exact on the single path; nll within its bound, +inf exactly without a
path, and in `uniform` also against the integer alignment count; the gradient stage against float64 on the device's own lattices, its
NaN mask the reference's (and so torch's), zeros under zero_infinity and past in_len; end to end against the composed bound.  Across
forms on the same input alpha, nll and the gradient are bit-identical, and every run is repeated once with the same bits.

CTCN_CTC_LOG=<file>: one JSON line per case and form with the worst error / bound ratios.
Measured on the MI355X (worst error / bound per kernel form over all its cases; asserted: <= 1; no kernel exceeded a bound):
  form                                   cases  utterances  alpha  beta   nll    gradient stage
  skewed 1 / 2 / 4 waves, side by side   2 each 32 each     0.45   0.48   0.08   0.93 (SEP)
  skewed, alpha alone                    2 each 32 each     0.45   -      0.08   -
  classic NS 1 (option off)              6      96          0.45   0.48   0.08   0.93 (SEP)
  classic NS 2 / 4                       2 each 32 each     0.33   0.44   0.19   0.96 (SEP)
  classic NS 8 / 16                      2 each 12 each     0.37   0.43   0.22   0.97 (SEP)
  in-place beta, NS 1 .. 16              7      92          0.37   -      0.22   0.97 (SEP = false)
  grad_ex none / mean / sum, zero_infinity on and off, middle blank   24   344   0.42   0.47   0.22   0.94
  log-softmax forward  5 cases, 135 rows: 0.49;  backward  7 cases, 2117 rows: 0.94
End-to-end max |dlp - float64| per regime: gauss 2.0e-2, aligned8 1.2e-5, aligned100 7e-46, aligned1e4 0, misaligned8 2.4e-3,
misaligned100 0.17, misaligned1e4 89 (a float32 ulp of the lattice is 0.5 there), uniform0 5.2e-5, uniformV 1.6e-2, shifted 2.7e-3,
single_path 2.2e-7, masked_classes 3.2e-3, blank_forbidden 5.1e-3, cut 8.0e-3.  The device's NaN mask is the reference's at every case.
The file takes 14 s, the slowest test 2 s.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
LMAXES = [s[0] for s in R.SHAPES]
RED = {"none": 0, "mean": 1, "sum": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _log(**rec):
    path = os.environ.get("CTCN_CTC_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec, sort_keys=True) + "\n")


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


_dev_cache = {}


def _on_device(dev, b):
    key = (b["Lmax"], b["blank"])
    if key not in _dev_cache:
        _dev_cache[key] = dict(lp=torch.from_numpy(b["lp"].copy()).to(dev).contiguous(), tg=torch.from_numpy(b["targets"]).to(dev).contiguous(),
                               il=torch.from_numpy(b["in_len"]).to(dev), tl=torch.from_numpy(b["tgt_len"]).to(dev))
    return _dev_cache[key]


def _fwd_ex(dev, b, with_beta, skew):
    """ctcn_ctc_fwd_ex into sentinel-filled buffers under ctc_lattice_skew = skew -> device alpha, beta, nll."""
    from ctc_pytorch_amd import _lib, ops
    d = _on_device(dev, b)
    alpha = torch.full((b["T"], b["B"], 2 * b["Lmax"] + 1), SENTINEL, device=dev)
    beta = torch.full_like(alpha, SENTINEL) if with_beta else None
    nll = torch.full((b["B"],), SENTINEL, device=dev)
    old = ops.get_option("ctc_lattice_skew")
    try:
        ops.set_option("ctc_lattice_skew", skew)
        _lib.check(_lib.lib().ctcn_ctc_fwd_ex(_P(d["lp"]), _P(d["tg"]), _P(d["il"]), _P(d["tl"]), _P(alpha), _P(beta), _P(nll), b["T"], b["B"],
                                              b["V"], b["Lmax"], b["blank"], _lib.stream_ptr()), "ctc_fwd_ex")
    finally:
        ops.set_option("ctc_lattice_skew", old)
    return alpha, beta, nll


def _grad_ex(dev, b, alpha, beta, nll, gscale, stride, reduction, zero_infinity):
    from ctc_pytorch_amd import _lib
    d = _on_device(dev, b)
    grad = torch.full_like(d["lp"], SENTINEL)
    _lib.check(_lib.lib().ctcn_ctc_grad_ex(_P(d["lp"]), _P(d["tg"]), _P(d["il"]), _P(d["tl"]), _P(alpha), _P(beta), _P(nll), _P(gscale), stride,
                                           RED[reduction], int(zero_infinity), b["blank"], _P(grad), b["T"], b["B"], b["V"], b["Lmax"],
                                           _lib.stream_ptr()), "ctc_grad_ex")
    return grad


def _side_by_side(dev, b, skew, reduction="sum", zero_infinity=False, g=None):
    """Form 2: ctcn_ctc_fwd_ex with beta + ctcn_ctc_grad_ex (SEP gradient) -> numpy alpha, beta, nll, dlp."""
    alpha, beta, nll = _fwd_ex(dev, b, True, skew)
    if g is None:
        gscale, stride = torch.ones(1, device=dev), 0
    else:
        gscale, stride = torch.from_numpy(np.asarray(g, dtype=np.float32)).to(dev), 1
    grad = _grad_ex(dev, b, alpha, beta, nll, gscale, stride, reduction, zero_infinity)
    torch.cuda.synchronize()
    return dict(alpha=alpha.cpu().numpy(), beta=beta.cpu().numpy(), nll=nll.cpu().numpy(), dlp=grad.cpu().numpy())


def _alpha_alone(dev, b, skew):
    """Form 1: ctcn_ctc_fwd_ex with beta = NULL."""
    alpha, _, nll = _fwd_ex(dev, b, False, skew)
    torch.cuda.synchronize()
    return dict(alpha=alpha.cpu().numpy(), nll=nll.cpu().numpy())


def _in_place(dev, b):
    """Form 3: ctcn_ctc_fwd + ctcn_ctc_bwd (blank 0): beta is added into alpha in place, SEP = false gradient."""
    from ctc_pytorch_amd import _lib
    assert b["blank"] == 0
    d = _on_device(dev, b)
    L, st = _lib.lib(), _lib.stream_ptr()
    alpha = torch.full((b["T"], b["B"], 2 * b["Lmax"] + 1), SENTINEL, device=dev)
    nll = torch.full((b["B"],), SENTINEL, device=dev)
    _lib.check(L.ctcn_ctc_fwd(_P(d["lp"]), _P(d["tg"]), _P(d["il"]), _P(d["tl"]), _P(alpha), _P(nll), b["T"], b["B"], b["V"], b["Lmax"], st), "ctc_fwd")
    a0 = alpha.clone()
    grad = torch.full_like(d["lp"], SENTINEL)
    gscale = torch.ones(1, device=dev)
    _lib.check(L.ctcn_ctc_bwd(_P(d["lp"]), _P(d["tg"]), _P(d["il"]), _P(d["tl"]), _P(alpha), _P(nll), _P(gscale), _P(grad), b["T"], b["B"], b["V"],
                              b["Lmax"], st), "ctc_bwd")
    torch.cuda.synchronize()
    return dict(alpha=a0.cpu().numpy(), ab=alpha.cpu().numpy(), nll=nll.cpu().numpy(), dlp=grad.cpu().numpy())


def _written_cells(res, b):
    """Exactly the cells t < in_len, s < 2 L + 1 of a lattice are written; the gradient is written whole."""
    for k in ("alpha", "beta", "ab"):
        if res.get(k) is None:
            continue
        a = res[k]
        for i in range(b["B"]):
            Tb, S = int(b["in_len"][i]), 2 * int(b["tgt_len"][i]) + 1
            assert (a[:Tb, i, :S] != SENTINEL).all(), (k, i)
            assert (a[Tb:, i, :] == SENTINEL).all() and (a[:, i, S:] == SENTINEL).all(), (k, i)
    assert (res["nll"] != SENTINEL).all()
    if res.get("dlp") is not None:
        assert not (res["dlp"] == SENTINEL).any()


_count_cache = {}


def _counted_nll(b, i):
    key = (b["Lmax"], b["blank"], i)
    if key not in _count_cache:
        u = b["utts"][i]
        _count_cache[key] = R.uniform_expectation(u["labels"], u["in_len"], b["blank"], b["V"], u["uniform_c"])[0]
    return _count_cache[key]


def _check_form(form, res, b, refs, gs=None, zero_infinity=False):
    """Every utterance of the batch through ctc_ref.check_utterance; gs: per-utterance float64 gradient scales (default 1)."""
    _written_cells(res, b)
    worst, e2e, fails = {}, {}, []
    for i, (u, r) in enumerate(zip(b["utts"], refs)):
        Tb, S = u["in_len"], 2 * len(u["labels"]) + 1
        got = {k: (res[k][:Tb, i, :S] if res.get(k) is not None else None) for k in ("alpha", "beta", "ab")}
        got["nll"] = res["nll"][i]
        got["dlp"] = res["dlp"][:, i] if res.get("dlp") is not None else None
        bad, ratio = R.check_utterance(u, r, got, 1.0 if gs is None else gs[i], zero_infinity)
        if "uniform_c" in u:
            want = _counted_nll(b, i)
            if abs(float(got["nll"]) - want) > R.nll_bound(r) + 1e-12 * abs(want):
                bad.append("nll:integer count")
        fails += ["%s %s" % (u["name"], x) for x in bad]
        for k, v in ratio.items():
            if k == "dlp_end_to_end":
                e2e[u["name"]] = v
            else:
                worst[k] = max(worst.get(k, 0.0), v)
    _log(form=form, Lmax=b["Lmax"], blank=b["blank"], B=b["B"], worst=worst, end_to_end=e2e, failed=fails)
    assert not fails, (form, b["Lmax"], b["blank"], fails, worst)
    return worst


def _assert_same(a, b, keys, what):
    for k in keys:
        assert _same(a[k], b[k]), "%s: %s differs in %d cells" % (what, k, int((_bits(a[k]) != _bits(b[k])).sum()))


@pytest.mark.parametrize("blank_at", ["first", "last"])
@pytest.mark.parametrize("Lmax", LMAXES)
def test_lattices_and_gradient_stage(dev, Lmax, blank_at):
    """Forms 1-3: alpha alone, alpha and beta side by side + the SEP gradient (skewed and classic where both exist), the in-place beta pass."""
    from ctc_pytorch_amd import ops
    V = [s[2] for s in R.SHAPES if s[0] == Lmax][0]
    blank = 0 if blank_at == "first" else V - 1
    b, refs = R.batch(Lmax, blank), R.batch_reference(Lmax, blank)
    plan = ops.ctc_lattice_plan(Lmax)
    assert ops.get_option("ctc_lattice_skew") == 1 and (plan["skewed"], plan["waves"], plan["ns"]) == R.PLANS[Lmax]
    skews = (1, 0) if plan["skewed"] else (1,)
    first = None
    for skew in skews:
        kind = "skewed%dw" % plan["waves"] if skew and plan["skewed"] else "classicNS%d" % (1 if plan["skewed"] else plan["ns"])
        both = _side_by_side(dev, b, skew)
        _check_form("fwd_ex+grad_ex/%s" % kind, both, b, refs)
        alone = _alpha_alone(dev, b, skew)
        _check_form("fwd_ex alpha/%s" % kind, alone, b, refs)
        _assert_same(both, alone, ("alpha", "nll"), "alpha alone against side by side, %s" % kind)
        _assert_same(both, _side_by_side(dev, b, skew), ("alpha", "beta", "nll", "dlp"), "rerun %s" % kind)
        _assert_same(alone, _alpha_alone(dev, b, skew), ("alpha", "nll"), "rerun alpha alone %s" % kind)
        if first is None:
            first = both
        else:
            _assert_same(first, both, ("alpha", "beta", "nll", "dlp"), "skewed against classic")
    if blank == 0:
        inpl = _in_place(dev, b)
        _check_form("fwd+bwd in place/classicNS%d" % (1 if plan["skewed"] else plan["ns"]), inpl, b, refs)
        _assert_same(first, inpl, ("alpha", "nll", "dlp"), "in place against side by side")
        live = first["alpha"] != SENTINEL
        assert _same((first["alpha"] + first["beta"])[live], inpl["ab"][live])
        _assert_same(inpl, _in_place(dev, b), ("alpha", "ab", "nll", "dlp"), "rerun in place")


MODES = (("none", False), ("mean", True), ("mean", False), ("sum", True))


@pytest.mark.parametrize("Lmax", LMAXES)
def test_ctcloss_through_autograd(dev, Lmax):
    """Form 4: nn.CTCLoss with a middle blank: 'none' under a non-constant upstream gradient, 'mean', zero_infinity on and off.  The direct
    calls with the same scale go through every check; autograd must give their bits."""
    from ctc_pytorch_amd import nn
    V = [s[2] for s in R.SHAPES if s[0] == Lmax][0]
    blank = V // 2
    b, refs = R.batch(Lmax, blank), R.batch_reference(Lmax, blank)
    d = _on_device(dev, b)
    B = b["B"]
    up = (0.5 + np.arange(B) / 4.0).astype(np.float32)
    for reduction, zi in MODES[:2] if Lmax >= 600 else MODES:
        g = up if reduction == "none" else None
        gs = [R.grad_scale(float(up[i]) if g is not None else 1.0, reduction, B, len(u["labels"])) for i, u in enumerate(b["utts"])]
        direct = _side_by_side(dev, b, 1, reduction, zi, g)
        _check_form("grad_ex %s zinf%d" % (reduction, zi), direct, b, refs, gs, zi)
        x = d["lp"].clone().requires_grad_(True)
        loss = nn.CTCLoss(blank=blank, reduction=reduction, zero_infinity=zi)(x, d["tg"], d["il"], d["tl"])
        loss.backward(torch.from_numpy(up).to(dev)) if reduction == "none" else loss.backward()
        assert _same(x.grad.cpu().numpy(), direct["dlp"]), (reduction, zi)
        out = loss.detach().cpu().numpy().astype(np.float64)
        nll = direct["nll"].astype(np.float64)
        if zi:
            nll = np.where(np.isinf(nll), 0.0, nll)
        Ls = np.maximum(b["tgt_len"], 1)
        if reduction == "none":
            assert _same(out.astype(np.float32), nll.astype(np.float32))
        else:
            want = float((nll / Ls).mean()) if reduction == "mean" else float(nll.sum())
            if np.isinf(want):
                assert out == want
            else:
                assert abs(float(out) - want) <= 2 * B * R.U * float(np.abs(nll / (Ls if reduction == "mean" else 1)).sum()) + 1e-30, (out, want)


def _softmax_inputs(V, seed):
    """27 rows (not a multiple of 4): 7 each peaked at M = 8, 100, 1e4 on 0.5 N(0,1), 5 Gaussian rows with three -inf logits, one row with a
    single finite logit."""
    rs = np.random.RandomState(seed)
    rows = []
    for M in (8.0, 100.0, 1e4):
        x = 0.5 * rs.standard_normal((7, V))
        x[np.arange(7), rs.randint(0, V, size=7)] += M
        rows.append(x)
    x = 2 * rs.standard_normal((5, V))
    for r in range(5):
        x[r, rs.choice(V, size=3, replace=False)] = -np.inf
    rows.append(x)
    one = np.full((1, V), -np.inf)
    one[0, V // 3] = 3.25
    rows.append(one)
    return np.concatenate(rows).astype(np.float32)


def _softmax_fwd(dev, x):
    from ctc_pytorch_amd import _lib
    xd = torch.from_numpy(x).to(dev)
    lp = torch.full_like(xd, SENTINEL)
    _lib.check(_lib.lib().ctcn_log_softmax_fwd(_P(xd), _P(lp), None, x.shape[0], x.shape[1], _lib.stream_ptr()), "log_softmax_fwd")
    torch.cuda.synchronize()
    return lp.cpu().numpy()


def _softmax_bwd(dev, lp, g):
    from ctc_pytorch_amd import _lib
    ld, gd = torch.from_numpy(np.array(lp)).to(dev), torch.from_numpy(np.array(g)).to(dev)
    dx = torch.full_like(ld, SENTINEL)
    _lib.check(_lib.lib().ctcn_log_softmax_bwd(_P(ld), _P(gd), _P(dx), lp.shape[0], lp.shape[1], _lib.stream_ptr()), "log_softmax_bwd")
    torch.cuda.synchronize()
    return dx.cpu().numpy()


def _check_softmax_bwd(what, dx, lp, g):
    want, bound = R.log_softmax_bwd64(lp, g), R.log_softmax_bwd_bound(lp, g)
    assert np.array_equal(np.isnan(dx), np.isnan(want)) and not np.isinf(dx).any(), what
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        ratio = float((np.abs(dx.astype(np.float64) - want)[fin] / bound[fin]).max())
    _log(form="log_softmax_bwd", case=what, rows=int(lp.shape[0]), V=int(lp.shape[1]), worst={"dx": ratio})
    assert ratio <= 1, (what, ratio)


@pytest.mark.parametrize("V", [20, 62, 64, 65, 300])
def test_log_softmax_pair(dev, V):
    x = _softmax_inputs(V, V)
    lp = _softmax_fwd(dev, x)
    want, bound = R.log_softmax64(x), R.log_softmax_bound(x)
    assert np.array_equal(np.isneginf(lp), np.isneginf(want)) and np.isfinite(lp[np.isfinite(want)]).all()
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        ratio = float((np.abs(lp.astype(np.float64) - want)[fin] / bound[fin]).max())
    _log(form="log_softmax_fwd", V=V, rows=int(x.shape[0]), worst={"lp": ratio})
    assert ratio <= 1, ratio
    assert lp[-1, V // 3] == 0 and np.signbit(lp[-1, V // 3]) == 0 and np.isneginf(np.delete(lp[-1], V // 3)).all()
    assert _same(lp, _softmax_fwd(dev, x))
    # backward on the device's own log-probs: a Gaussian upstream gradient, one row with a NaN in it
    g = np.random.RandomState(V + 1).standard_normal(lp.shape).astype(np.float32)
    g[3, V // 2] = np.nan
    dx = _softmax_bwd(dev, lp, g)
    _check_softmax_bwd("V%d" % V, dx, lp, g)
    assert np.isnan(dx[3]).all() and _same(dx, _softmax_bwd(dev, lp, g))


@pytest.mark.parametrize("Lmax", LMAXES[:2])
def test_log_softmax_backward_on_the_loss_gradient(dev, Lmax):
    """ctcn_log_softmax_bwd on the regimes' log-probs and the device's own CTC gradient, its NaN rows included."""
    b = R.batch(Lmax, 0)
    res = _side_by_side(dev, b, 1)
    lp, g = b["lp"].reshape(-1, b["V"]), res["dlp"].reshape(-1, b["V"])
    assert np.isnan(g).any() and lp.shape[0] % 4 == 0
    lp, g = lp[:-1], g[:-1]                                                       # a row count that is no multiple of 4
    _check_softmax_bwd("loss gradient Lmax%d" % Lmax, _softmax_bwd(dev, lp, g), lp, g)


@pytest.mark.parametrize("Lmax", LMAXES)
def test_forced_alignment_on_known_paths(dev, Lmax):
    from ctc_pytorch_amd import ops
    b, refs = R.batch(Lmax, 0), R.batch_reference(Lmax, 0)
    d = _on_device(dev, b)
    res = ops.ctc_forced_align(d["lp"], d["tg"], d["il"], d["tl"], blank=0)
    paths, scores, ok = res.paths.cpu().numpy(), res.scores.cpu().numpy(), res.ok.cpu().numpy()
    for i, (u, r) in enumerate(zip(b["utts"], refs)):
        assert bool(ok[i]) == u["feasible"], u["name"]
        if "path" in u and u["feasible"]:
            assert np.array_equal(paths[i, :u["in_len"]], r["ext"][u["path"]])
            assert _same(scores[i:i + 1], np.array([-r["nll"]], dtype=np.float32))
        if "cut" in u:
            tc, s = u["cut"]
            assert paths[i, tc] == r["ext"][s]
        if not u["feasible"]:
            assert np.isneginf(scores[i])
