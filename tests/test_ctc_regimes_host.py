"""What tests/test_ctc_regimes.py rests on, checked without a GPU (no gpu marker): the float64 CTC reference of tests/ctc_ref.py against
torch's float64 CPU loss and against an exact integer alignment count, the regimes against what their names promise, the float32
emulation of the kernels' formulas inside every bound at every case of the GPU table, and every mutant of that emulation caught.

Measured (the assertions are the conditions; these are the figures behind them).
  reference against torch float64 (31 cases: the three small shapes x blanks 0, V - 1, V / 2 x none / sum / mean, the four larger shapes once
  each): nll within 1.2e-16 relative, gradient cells within 8.9e-16 of their yardstick (asserted: 1e-12), NaN mask and +inf pattern identical.
  reference against the integer count (uniform0, uniformV at every shape): nll and posteriors within 1e-12.
  float32 emulation, worst error / bound over the seven shapes (asserted: <= 1), and its distance from float64 end to end:
    regime           alpha  beta   nll     gradient stage   end-to-end max |dlp - float64|
    gauss            0.21   0.28   0.007   0.87             1.2e-2 (T 2250), 6.8e-6 (T 24)
    aligned 8        0.28   0.28   4e-4    0.35             1.2e-5
    aligned 100/1e4  0.33   0.33   0       7e-9             7e-46 / 0
    misaligned 8     0.30   0.26   0.030   0.90             8.2e-4
    misaligned 100   0.37   0.43   0.005   0.97             0.13 (T 2250, L 1100)
    misaligned 1e4   0.33   0.48   0.009   0.88             89 (a float32 ulp of the lattice is 0.5 there: only lattices and nll mean anything)
    uniform 0 / -lnV 0.24   0.24   0.22    0.91             6.7e-3
    shifted          0.26   0.21   0.040   0.80             1.5e-3
    single_path      0.25   0.14   0       0.19             4.3e-8 (lattice ratios: the cells off the path; on it, bit-exact)
    one_short, wall  0.27   0.20   -       0                - (all NaN, or zeros)
    masked_classes   0.27   0.20   0.079   0.80             1.6e-3
    blank_forbidden  0.21   0.24   0.044   0.76             1.7e-3
    cut              0.22   0.21   0.013   0.85             4.3e-3
  The gradient stage's 0.97 is the single rounding of lcab = fl(m + logf(s)) at |lcab| = 1.34e5, just above 2^17, where half an ulp is
  0.98 u |lcab|: the bound's leading term is attained, not exceeded.
  Each of the thirteen mutants (the prefetch-edge fault as two: frame 4 and the last frame) breaks a claim at the row CAUGHT_BY names.
  The file takes 19 s.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_ref as R  # noqa: E402

LMAXES = [s[0] for s in R.SHAPES]
SMALL = LMAXES[:3]


def _blanks(V):
    return (0, V - 1, V // 2)


def _torch_cases():
    out = []
    for Lmax, _, V, _ in R.SHAPES:
        if Lmax in SMALL:                                             # every regime, three blanks, three reductions, zero_infinity both ways
            for bi, blank in enumerate(_blanks(V)):
                for ri, red in enumerate(("none", "sum", "mean")):
                    out.append((Lmax, blank, red, (bi + ri + Lmax) % 2 == 0))
        else:                                                         # the larger rows once each, the modes in turn
            i = LMAXES.index(Lmax)
            out.append((Lmax, _blanks(V)[i % 3], ("none", "sum", "mean")[i % 3], i % 2 == 0))
    return out


def _upstream(B):
    return 0.5 + np.arange(B) / 4.0                                   # a non-constant upstream gradient for 'none'


@pytest.mark.parametrize("Lmax,blank,reduction,zero_infinity", _torch_cases())
def test_reference_matches_torch_float64(Lmax, blank, reduction, zero_infinity):
    """nll and every finite gradient cell of the reference against torch.nn.functional.ctc_loss in float64 on the CPU; the NaN mask and the
    +inf pattern identical.  The yardstick for a cell is 1e-12 of max(1, |value|) times the largest magnitude of the utterance's lattice: a
    posterior is the exponential of a difference of lattice values, so float64's own resolution of those values (1.1e-16 of up to 4e6 per
    step in misaligned(1e4)) is what either side can know of it.  Measured: 8.9e-16 of that yardstick at worst, i.e. four float64 ulps of
    the lattice.  (1e-12 of max(1, |value|) alone is met by nll everywhere, but not by two float64 gradients at these sizes: torch and the
    reference differ by 9.4e-12 in gauss at T = 2250 and by 4.7e-10 in misaligned(1e4) at T = 640.)"""
    b = R.batch(Lmax, blank)
    refs = R.batch_reference(Lmax, blank)
    B, T = b["B"], b["T"]
    lp = torch.from_numpy(b["lp"].astype(np.float64)).requires_grad_(True)
    tg, il, tl = (torch.from_numpy(b[k]) for k in ("targets", "in_len", "tgt_len"))
    with torch.no_grad():
        nll_t = TF.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=False).numpy()
    loss = TF.ctc_loss(lp, tg, il, tl, blank=blank, reduction=reduction, zero_infinity=zero_infinity)
    g = _upstream(B) if reduction == "none" else np.ones(B)
    loss.backward(torch.from_numpy(g)) if reduction == "none" else loss.backward()
    grad_t = lp.grad.numpy()
    worst_nll = worst_g = 0.0
    for i, (u, r) in enumerate(zip(b["utts"], refs)):
        assert np.isinf(nll_t[i]) == (r["nll"] == np.inf) == (not u["feasible"]), (u["name"], nll_t[i], r["nll"])
        if u["feasible"]:
            worst_nll = max(worst_nll, abs(nll_t[i] - r["nll"]) / max(1.0, abs(r["nll"])))
        want = R.ref_dlp(r, u["lp"], R.grad_scale(g[i], reduction, B, len(u["labels"])), zero_infinity)
        got = grad_t[:, i]
        assert np.array_equal(np.isnan(got), np.isnan(want)), u["name"]
        assert not np.isinf(got).any() and not np.isinf(want).any(), u["name"]
        lpn = u["lp"].astype(np.float64)
        nan_lp = np.isnan(want) & (np.arange(T) < u["in_len"])[:, None]
        if u["feasible"]:                                             # NaN exactly at the -inf log-probs of the utterance's frames
            assert np.array_equal(nan_lp, np.isneginf(lpn) & (np.arange(T) < u["in_len"])[:, None]), u["name"]
        fin = np.isfinite(want)
        mag = max(1.0, float(np.abs(r["ab"][np.isfinite(r["ab"])]).max()) if np.isfinite(r["ab"]).any() else 1.0)
        scale = np.maximum(1.0, np.abs(want)) * mag
        worst_g = max(worst_g, float((np.abs(got - want)[fin] / scale[fin]).max()))
    print("torch parity Lmax %d blank %d %s zinf %d: nll %.2e  gradient %.2e" % (Lmax, blank, reduction, zero_infinity, worst_nll, worst_g))
    assert worst_nll <= 1e-12 and worst_g <= 1e-12


@pytest.mark.parametrize("Lmax", LMAXES)
def test_reference_matches_the_integer_count(Lmax):
    b = R.batch(Lmax)
    seen = 0
    for u, r in zip(b["utts"], R.batch_reference(Lmax)):
        if "uniform_c" not in u:
            continue
        seen += 1
        nll, post = R.uniform_expectation(u["labels"], u["in_len"], 0, b["V"], u["uniform_c"])
        assert abs(nll - r["nll"]) <= 1e-12 * max(1.0, abs(nll)), (u["name"], nll, r["nll"])
        assert float(np.abs(post - r["post"]).max()) <= 1e-12, u["name"]
        assert float(np.abs(post.sum(axis=1) - 1).max()) <= 1e-12
    assert seen >= 1


@pytest.mark.parametrize("Lmax", LMAXES)
def test_single_path_and_one_short(Lmax):
    b = R.batch(Lmax)
    refs = R.batch_reference(Lmax)
    names = [u["name"] for u in b["utts"]]
    u, r = b["utts"][names.index("single_path")], refs[names.index("single_path")]
    fin = np.isfinite(r["ab"])
    assert (fin.sum(axis=1) == 1).all() and np.array_equal(np.argmax(fin, axis=1), u["path"])
    assert R.count_alignments(u["labels"], u["in_len"], 0, b["V"])[0] == 1
    t = np.arange(u["in_len"])
    run = np.cumsum(u["lp"].astype(np.float64)[t, r["ext"][u["path"]]])
    assert np.array_equal(r["alpha"][t, u["path"]], run) and r["nll"] == -run[-1]          # exact running sums, in float32 too:
    assert np.array_equal(run.astype(np.float32).astype(np.float64), run) and abs(run[-1]) * 64 < 2 ** 24
    if "one_short" in names:
        u1, r1 = b["utts"][names.index("one_short")], refs[names.index("one_short")]
        assert r1["nll"] == np.inf and not np.isfinite(r1["ab"]).any()
        assert R.count_alignments(u1["labels"], u1["in_len"], 0, b["V"])[0] == 0
        assert u1["in_len"] == R.min_frames(u1["labels"]) - 1


@pytest.mark.parametrize("Lmax", LMAXES)
def test_regimes_are_what_they_say(Lmax):
    b = R.batch(Lmax)
    assert b["tgt_len"].max() == Lmax and b["in_len"].max() == b["T"] and (b["in_len"] >= 1).all()
    for u, r in zip(b["utts"], R.batch_reference(Lmax)):
        name, Tb, lp = u["name"], u["in_len"], u["lp"].astype(np.float64)[:u["in_len"]]
        dead = 1.0 - np.isfinite(r["ab"]).mean()
        L = len(u["labels"])
        assert L == 0 or 0.1 <= R.repeats(u["labels"]) / max(L - 1, 1) <= 0.45 or L < 12, (name, R.repeats(u["labels"]), L)
        assert (r["nll"] != np.inf) == u["feasible"], name
        if name.startswith("aligned"):
            assert (lp.max(axis=1) > (-1e-30 if u["M"] >= 100 else -0.1)).all(), name
            assert 0 <= r["nll"] <= (1e-30 if u["M"] >= 100 else 0.05 * Tb), (name, r["nll"])
        elif name.startswith("misaligned"):
            assert r["nll"] > 0.25 * u["M"] * Tb, (name, r["nll"])
            assert np.abs(r["alpha"][np.isfinite(r["alpha"])]).max() > 0.25 * u["M"] * Tb
        elif name == "shifted":
            assert np.exp(lp).max() > 1 and np.abs(R._lse_rows(lp, 1)).max() > 4
        elif name == "single_path":
            assert np.isfinite(r["ab"]).sum() == Tb and dead > 0.9
        elif name in ("one_short", "wall"):
            assert dead == 1.0 and np.isfinite(r["alpha"]).any() and np.isfinite(r["beta"]).any()
        elif name == "masked_classes":
            assert np.isneginf(lp[:, u["masked"]]).all() and not set(u["masked"]) & set(u["labels"].tolist())
        elif name == "blank_forbidden":
            assert np.isneginf(lp[u["forbidden"], 0]).all() and len(u["forbidden"]) == Tb // 3
        elif name == "cut":
            tc, s = u["cut"]
            assert np.isfinite(r["ab"][tc]).sum() == 1 and np.isfinite(r["ab"][tc, s]) and (u["labels"] == r["ext"][s]).sum() == 1
            assert np.isfinite(lp[tc]).sum() == 1 and lp[tc].max() == 0


_ratios = {}


@pytest.mark.parametrize("Lmax", LMAXES)
def test_emulation_is_inside_every_bound(Lmax):
    """A correct float32 implementation meets every claim the GPU test makes, at every utterance of its table: the bounds are attainable."""
    b = R.batch(Lmax)
    for u, r in zip(b["utts"], R.batch_reference(Lmax)):
        e = R.emulate(u["lp"], u["labels"], u["in_len"], 0)
        bad, ratio = R.check_utterance(u, r, e)
        assert not bad, (Lmax, u["name"], bad, ratio)
        for k, v in ratio.items():
            key = (u["name"].rstrip("0123456789e"), k) if k != "dlp_end_to_end" else (u["name"], k)
            _ratios[key] = max(_ratios.get(key, 0.0), v)
    if Lmax == LMAXES[-1]:
        for key in sorted(_ratios):
            print("emulation %-16s %-15s %.3g" % (key + (_ratios[key],)))


def test_emulation_modes():
    """'mean', 'none' with an upstream gradient, zero_infinity and a blank other than 0 through the same checks."""
    for blank, red, zi in ((19, "mean", False), (10, "none", True), (0, "mean", True)):
        b = R.batch(40, blank)
        g = _upstream(b["B"])
        for i, (u, r) in enumerate(zip(b["utts"], R.batch_reference(40, blank))):
            gi = float(np.float32(g[i])) if red == "none" else 1.0
            e = R.emulate(u["lp"], u["labels"], u["in_len"], blank, g=gi, reduction=red, B=b["B"], zero_infinity=zi)
            bad, _ = R.check_utterance(u, r, e, R.grad_scale(gi, red, b["B"], len(u["labels"])), zi)
            assert not bad, (blank, red, zi, u["name"], bad)


# mutant -> the row (Lmax, regime) that catches it, and the claim it breaks there
CAUGHT_BY = {
    "skip_equal": (40, "gauss", "alpha:-inf pattern"),
    "beta_skip_back": (40, "gauss", "beta:-inf pattern"),
    "nll_last_state": (40, "gauss", "nll:bound"),
    "seed_state0": (40, "single_path", "alpha:-inf pattern"),
    "beta_seed_T": (40, "shifted", "beta:-inf pattern"),
    "pf_frame4": (40, "single_path", "alpha:single path bits"),
    "pf_last": (40, "single_path", "nll:single path bits"),
    "first_position": (40, "uniformV", "dlp:stage bound"),
    "blank_no_2L": (40, "uniform0", "dlp:stage bound"),
    "lse_max": (40, "uniformV", "alpha:bound"),
    "lse_drop_min": (40, "uniformV", "alpha:bound"),
    "wave_edge64": (40, "misaligned100", "alpha:-inf pattern"),
    "mean_by_L": (40, "aligned8", "dlp:stage bound"),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught(mutant):
    Lmax, regime, claim = CAUGHT_BY[mutant]
    b = R.batch(Lmax)
    i = [u["name"] for u in b["utts"]].index(regime)
    u, r = b["utts"][i], R.batch_reference(Lmax)[i]
    red = "mean" if mutant == "mean_by_L" else "sum"
    gs = R.grad_scale(1.0, red, b["B"], len(u["labels"]))
    assert not R.check_utterance(u, r, R.emulate(u["lp"], u["labels"], u["in_len"], 0, reduction=red, B=b["B"]), gs)[0]
    bad, ratio = R.check_utterance(u, r, R.emulate(u["lp"], u["labels"], u["in_len"], 0, reduction=red, B=b["B"], mutant=mutant), gs)
    print("mutant %-15s at Lmax %d %-14s breaks %s" % (mutant, Lmax, regime, bad))
    assert claim in bad, (mutant, bad, ratio)
