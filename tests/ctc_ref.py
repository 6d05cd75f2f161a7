"""CTC loss references for the kernels of ctc.hip outside the Gaussian regime (numpy only; tests/test_ctc_regimes_host.py checks this
file on the CPU, tests/test_ctc_regimes.py holds the kernels to it).

What is here
  reference(lp, labels, in_len, blank)  float64 log-domain CTC of ONE utterance: alpha, beta (beta includes the frame's own log-prob, as
                          the kernels' does, so alpha + beta = log(mass through the cell) + lp), nll, the class occupancies lcab and the
                          posteriors exp(lcab + nll - lp).  -inf follows IEEE through the kernels' formulas: a dead cell is exactly -inf,
                          nll = +inf without a path, and ref_dlp is NaN exactly where exp(lcab + nll - l) meets -inf - (-inf) or -inf + inf.
  log_softmax64 / log_softmax_bwd64     float64 log-softmax, forward and backward.
  count_alignments        the same recursion over Python integers: N alignments, N[t, c] of them through class c at frame t.
  emulate                 a float32 restatement of the kernels' FORMULAS (not their code): lse3 as max, three exp2((x - m) log2e),
                          m + log2(sum) ln2, then + q; the gradient as an online log-sum-exp over a class's positions, then
                          exp(l) - exp(lcab + n - l).  exp2 / log2 / exp / log are the float64 functions rounded to float32 (at most an
                          ulp from the truth, and the same on every machine).  MUTANTS names its deliberately wrong variants.
  bounds                  lattice_bound, nll_bound, grad_stage, composed_grad_bound, log_softmax_bound, log_softmax_bwd_bound (derivations below).
  regimes                 one seeded utterance each (REGIMES), batch() puts them together for the shapes of SHAPES.

Error bounds.  u = 2^-24 (float32 unit roundoff; one ulp of a function result is a relative error of at most 2 u).  Every bound is
computed from float64 reference values and these unit errors; no device result enters a lattice, nll or log-softmax bound, and the
gradient stage is judged on its own inputs (below).

(1) One lse3.  m is exact.  d_i = fl(x_i - m) (relative u), p_i = fl(d_i * fl(log2 e)) (constant and product: 2 u more), so the
    exponent is off by at most 3 u |d_i| in natural units and the term e^{d_i} by 3 u |d_i| e^{d_i} <= 3 u / e = 1.11 u; exp2 (1 ulp)
    adds 2 u e^{d_i} <= 2 u.  The maximum's own term is exp2(0) = 1 exactly, so two terms carry 2 * 3.11 u = 6.21 u.  fl(1 + t1) <= 2
    rounds by at most u, the second add (<= 3) by 2 u: the sum in [1, 3] is off by 9.21 u absolute, hence relative, and so is its
    logarithm.  log2 (1 ulp of a result below 2): 2 u, times ln 2 = 1.39 u; fl(ln 2) and the product: 2 u * 1.0986 = 2.2 u.
    e = 9.21 + 1.39 + 2.2 = 12.8 u, taken as E_LSE3 = 13 u = 7.7e-7.
(2) A lattice cell.  lse3 is a log of a positive combination, so it moves by at most the largest error of its operands: the errors of
    the frames add.  Per frame: e, the rounding of m + r (u |lse3| <= u (A_t + Q_t)) and of + q (u A_t).  With A_t = max |finite
    lattice value| and Q_t = max |finite gathered log-prob| of the frame, b_t = b_{t-1} + e + u (2 (A_t + b_{t-1}) + Q_t), b = 0 at the
    pass's first frame (a copy); the b_{t-1} inside is the device's own magnitude.  One bound per frame, for all its cells.
(3) nll = -(m + log(e^{l1 - m} + e^{l2 - m})) from the last frame: b_{T-1} for its operands, 0.37 u + 2 u for the one inexact term,
    u for the add (<= 2), u for log (1 ulp of a result below ln 2 < 1), together under 5 u, and u |nll| for the last add.
(4) The gradient stage on its own inputs: the test takes the device's float32 alpha, beta, nll, forms ab = fl(alpha + beta) as the
    kernel does and evaluates lcab* = logsumexp_j ab, p* = exp(lcab* + n - l), g* = (e^l - p*) gs in float64.  The kernel's lcab sums
    k terms by an online log-sum-exp: one step is fl(s + expf(fl(x - m))) or fl(fl(s expf(fl(m - x))) + 1); relative to the running
    sum (>= 1) the first costs 0.37 u + 2 u + u, the second (u |d| + 3 u) s e^d / (s e^d + 1) <= (ln k + 3) u, both under
    (4 + ln(k + 1)) u.  The blank's wave-wide variant does ceil(k / 64) such steps per lane, one rescaling and a 6-level tree: under 8
    further steps.  So the sum is off by at most (k + 8)(4 + ln(k + 1)) u relative; logf adds 2 u max(1, ln k), the add u |lcab|,
    fl(lcab + n) u |lcab + n|, fl(. - l) u |lcab + n - l|, the last expf 2 u:
        delta = u (|lcab| + |lcab + n| + |lcab + n - l| + 2 max(1, ln k) + (k + 8)(4 + ln(k + 1)) + 2)        (c' = 6 in |.|max terms)
    and |g - g*| <= |gs| (p* expm1(delta) + 5 u max(e^l, p*)) + 1e-37: expf(l) 2 u, the subtraction u, the product with gs u, the
    division behind 'mean' u (c = 5); 1e-37 covers results flushed below the normal range.
(5) End to end the same form holds with delta + the two lattice bounds of the frame + u |alpha + beta| + the nll bound in the
    exponent (composed_grad_bound): loose at large magnitudes, where float32's own end-to-end error is large.
(6) log-softmax forward: lanes sum ceil(V / 64) terms each, then a 6-level tree: the sum (>= 1) is off by (ceil(V / 64) + 6) u from
    the adds and 0.37 u + 2 u from a term; logf 2 u max(1, ln V); fl(m + .) u |lse|; fl(x - lse) u |lp|.  Backward g - e^l sum(g):
    the sum is off by (ceil(V / 64) + 6) u sum|g|, expf 2 u, the product u, the subtraction u |dx|.
"""
import math

import numpy as np

U = 2.0 ** -24
E_LSE3 = 13 * U
F = np.float32
NINF = -np.inf
_L2E = F(1.4426950408889634)
_LN2 = F(0.6931471805599453)
_quiet = dict(all="ignore")


# ---------------------------------------------------------------------------------------------------------------------------------
# the lattice's static structure
# ---------------------------------------------------------------------------------------------------------------------------------
def ext_labels(labels, blank):
    labels = np.asarray(labels, dtype=np.int64)
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    return ext


def skip_masks(ext):
    """(alpha's, beta's) skip rule: a label state may skip the blank between two different labels."""
    S = len(ext)
    fa, fb = np.zeros(S, dtype=bool), np.zeros(S, dtype=bool)
    odd = (np.arange(S) & 1) == 1
    fa[2:] = odd[2:] & (ext[2:] != ext[:-2])
    fb[:-2] = odd[:-2] & (ext[:-2] != ext[2:])
    return fa, fb


def _shift(a, k, fill=NINF):
    """out[s] = a[s - k] (k > 0: the lower neighbours, alpha) or a[s + |k|] (k < 0, beta)."""
    out = np.full_like(a, fill)
    if k > 0:
        out[k:] = a[:-k]
    else:
        out[:k] = a[-k:]
    return out


def repeats(labels):
    labels = np.asarray(labels)
    return int((labels[1:] == labels[:-1]).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _lse_rows(x, axis):
    """logsumexp along an axis; all -inf -> -inf."""
    with np.errstate(**_quiet):
        m = x.max(axis=axis, keepdims=True)
        m0 = np.where(np.isfinite(m), m, 0.0)
        return (m0 + np.log(np.exp(x - m0).sum(axis=axis, keepdims=True))).squeeze(axis)


def _lse3_64(x0, x1, x2):
    return _lse_rows(np.stack([x0, x1, x2]), 0)


def reference(lp, labels, in_len, blank):
    """lp (T, V) (any float type, widened exactly), labels (L,), in_len >= 1.  Returns a dict: alpha, beta, ab (in_len, S), nll, lcab and
    post (in_len, V), q (the gathered log-probs), ext."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb = int(in_len)
    ext = ext_labels(labels, blank)
    S = len(ext)
    fa, fb = skip_masks(ext)
    q = lp[:Tb][:, ext]
    alpha = np.full((Tb, S), NINF)
    beta = np.full((Tb, S), NINF)
    alpha[0, :2] = q[0, :2]
    beta[Tb - 1, max(S - 2, 0):] = q[Tb - 1, max(S - 2, 0):]
    with np.errstate(**_quiet):
        for t in range(1, Tb):
            a = alpha[t - 1]
            alpha[t] = _lse3_64(a, _shift(a, 1), np.where(fa, _shift(a, 2), NINF)) + q[t]
        for t in range(Tb - 2, -1, -1):
            b = beta[t + 1]
            beta[t] = _lse3_64(b, _shift(b, -1), np.where(fb, _shift(b, -2), NINF)) + q[t]
        tot = _lse_rows(alpha[Tb - 1, max(S - 2, 0):], 0)
        nll = np.inf if tot == NINF else -float(tot)
        ab = alpha + beta
        V = lp.shape[1]
        lcab = np.full((Tb, V), NINF)
        for c in np.unique(ext):
            lcab[:, c] = _lse_rows(ab[:, ext == c], 1)
        post = np.exp(lcab + nll - lp[:Tb])
    return dict(alpha=alpha, beta=beta, ab=ab, nll=nll, lcab=lcab, post=post, q=q, ext=ext)


def grad_scale(g, reduction, B, L):
    return g / (B * max(L, 1)) if reduction == "mean" else g


def ref_dlp(ref, lp, gs=1.0, zero_infinity=False):
    """(T, V) float64: (exp(lp) - posterior) gs on the frames of the utterance, zeros past them; zeros for an infeasible utterance under
    zero_infinity, NaN rows otherwise (the formula's own)."""
    lp = np.asarray(lp, dtype=np.float64)
    out = np.zeros_like(lp)
    Tb = ref["post"].shape[0]
    if not (zero_infinity and ref["nll"] == np.inf):
        with np.errstate(**_quiet):
            out[:Tb] = (np.exp(lp[:Tb]) - ref["post"]) * gs
    return out


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(**_quiet):
        return x - _lse_rows(x, -1)[..., None]


def log_softmax_bwd64(lp, g):
    lp, g = np.asarray(lp, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(**_quiet):
        return g - np.exp(lp) * g.sum(axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact alignment counter
# ---------------------------------------------------------------------------------------------------------------------------------
def count_alignments(labels, in_len, blank, V):
    """N = number of frame-level alignments of the label string over in_len frames, Ntc (in_len, V) = how many of them emit class c at
    frame t; Python integers throughout (object arrays), only the reachable band of states is touched."""
    Tb = int(in_len)
    ext = ext_labels(labels, blank)
    S = len(ext)
    fa, fb = (m.astype(object) for m in skip_masks(ext))
    A = np.zeros((Tb, S + 2), dtype=object)            # two zero columns in front (alpha) ...
    Bt = np.zeros((Tb, S + 2), dtype=object)           # ... and behind (beta)
    A[0, 2] = 1
    if S > 1:
        A[0, 3] = 1
    Bt[Tb - 1, S - 1] = 1
    if S > 1:
        Bt[Tb - 1, S - 2] = 1
    for t in range(1, Tb):
        lo, hi = max(0, S - 2 * (Tb - t)), min(S, 2 * t + 2)
        if lo < hi:
            p = A[t - 1]
            A[t, lo + 2:hi + 2] = p[lo + 2:hi + 2] + p[lo + 1:hi + 1] + fa[lo:hi] * p[lo:hi]
    for t in range(Tb - 2, -1, -1):
        lo, hi = max(0, S - 2 * (Tb - t)), min(S, 2 * t + 2)
        if lo < hi:
            p = Bt[t + 1]
            Bt[t, lo:hi] = p[lo:hi] + p[lo + 1:hi + 1] + fb[lo:hi] * p[lo + 2:hi + 2]
    A, Bt = A[:, 2:], Bt[:, :S]
    N = A[Tb - 1, S - 1] + (A[Tb - 1, S - 2] if S > 1 else 0)
    through = A * Bt
    Ntc = np.zeros((Tb, V), dtype=object)
    for c in np.unique(ext):
        Ntc[:, c] = through[:, ext == c].sum(axis=1)
    return int(N), Ntc


def uniform_expectation(labels, in_len, blank, V, c):
    """lp == c everywhere: nll = -(T c + ln N), posterior N[t, c] / N; nothing shared with `reference`."""
    N, Ntc = count_alignments(labels, in_len, blank, V)
    if N == 0:
        return np.inf, None
    post = np.array([[float(x / N) if x else 0.0 for x in row] for row in Ntc])        # int / int: correctly rounded
    return -(int(in_len) * float(c) + math.log(N)), post


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' formulas, and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("skip_equal", "beta_skip_back", "nll_last_state", "seed_state0", "beta_seed_T", "pf_frame4", "pf_last", "first_position",
           "blank_no_2L", "lse_max", "lse_drop_min", "wave_edge64", "mean_by_L")


def _f(fn, x):
    """a float32 function: the float64 one, rounded."""
    with np.errstate(**_quiet):
        return fn(np.asarray(x, dtype=np.float64)).astype(F)


def _lse3_32(x0, x1, x2, mutant):
    with np.errstate(**_quiet):
        m = np.maximum(x0, np.maximum(x1, x2))
        if mutant == "lse_max":
            r = m
        else:
            e = [_f(np.exp2, (x - m) * _L2E) for x in (x0, x1, x2)]
            if mutant == "lse_drop_min":
                lo = np.minimum(e[0], np.minimum(e[1], e[2]))
                s = (e[0] + e[1]) + e[2] - lo
            else:
                s = (e[0] + e[1]) + e[2]
            r = m + _f(np.log2, s) * _LN2
        return np.where(m == NINF, F(NINF), r).astype(F)


def emulate_grad_stage(lp, ab, nll, labels, blank, gs, mutant=None):
    """float32: lp (Tb, V), ab (Tb, S) = alpha + beta, nll, gs scalars -> (Tb, V)."""
    lp, ab = np.asarray(lp, dtype=F), np.asarray(ab, dtype=F)
    Tb, V = lp.shape
    L = len(labels)
    m = np.full((Tb, V), NINF, dtype=F)
    s = np.zeros((Tb, V), dtype=F)

    def add(c, x):
        with np.errstate(**_quiet):
            mc, sc = m[:, c].copy(), s[:, c].copy()
            up = x > mc
            s_up = sc * _f(np.exp, mc - x) + F(1)
            s_in = sc + _f(np.exp, x - mc)
            dead = x == NINF
            s[:, c] = np.where(dead, sc, np.where(up, s_up, s_in))
            m[:, c] = np.where(dead | ~up, mc, x)

    for j in range(L + (0 if mutant == "blank_no_2L" else 1)):
        add(blank, ab[:, 2 * j])
    seen = set()
    for j in range(L):
        c = int(labels[j])
        if mutant == "first_position" and c in seen:
            continue
        seen.add(c)
        add(c, ab[:, 2 * j + 1])
    with np.errstate(**_quiet):
        lcab = np.where(m == NINF, F(NINF), m + _f(np.log, s)).astype(F)
        arg = (lcab + F(nll)) - lp
        return ((_f(np.exp, lp) - _f(np.exp, arg)) * F(gs)).astype(F)


def emulate(lp, labels, in_len, blank, g=1.0, reduction="sum", B=1, zero_infinity=False, mutant=None):
    """The float32 stand-in for one utterance: lp (T, V) float32 (all T rows of the tensor), -> dict alpha, beta (in_len, S), nll, dlp (T, V)."""
    lp = np.asarray(lp, dtype=F)
    T, V = lp.shape
    Tb, L = int(in_len), len(labels)
    ext = ext_labels(labels, blank)
    S = len(ext)
    fa, fb = skip_masks(ext)
    if mutant == "skip_equal":
        odd = (np.arange(S) & 1) == 1
        fa, fb = odd & (np.arange(S) >= 2), odd & (np.arange(S) + 2 < S)
    if mutant == "beta_skip_back":
        fb = np.zeros(S, dtype=bool)
        for s_ in range(1, S - 2, 2):
            fb[s_] = ext[s_] != ext[s_ - 2] if s_ >= 2 else True
    q = lp[:, ext]
    alpha = np.full((Tb, S), NINF, dtype=F)
    alpha[0, 0] = q[0, 0]
    if S > 1 and mutant != "seed_state0":
        alpha[0, 1] = q[0, 1]
    for t in range(1, Tb):
        tq = t
        if mutant == "pf_frame4" and t == 4 and Tb > 5:
            tq = 5
        if mutant == "pf_last" and t == Tb - 1:
            tq = t - 1
        a = alpha[t - 1]
        x1 = _shift(a, 1)
        if mutant == "wave_edge64" and S > 64:
            x1[64] = NINF
        with np.errstate(**_quiet):
            alpha[t] = _lse3_32(a, x1, np.where(fa, _shift(a, 2), F(NINF)), mutant) + q[tq]
    t_last = T - 1 if mutant == "beta_seed_T" else Tb - 1
    beta = np.full((t_last + 1, S), NINF, dtype=F)
    beta[t_last, max(S - 2, 0):] = q[t_last, max(S - 2, 0):]
    for t in range(t_last - 1, -1, -1):
        b = beta[t + 1]
        with np.errstate(**_quiet):
            beta[t] = _lse3_32(b, _shift(b, -1), np.where(fb, _shift(b, -2), F(NINF)), mutant) + q[t]
    beta = beta[:Tb]
    l1 = alpha[Tb - 1, S - 1]
    l2 = alpha[Tb - 1, S - 2] if S > 1 and mutant != "nll_last_state" else F(NINF)
    mx = max(l1, l2)
    with np.errstate(**_quiet):
        nll = F(np.inf) if mx == NINF else F(-(mx + _f(np.log, _f(np.exp, l1 - mx) + _f(np.exp, l2 - mx))))
    gs = F(g)
    if reduction == "mean":
        gs = gs / (F(max(L, 1)) if mutant == "mean_by_L" else F(B) * F(max(L, 1)))
    dlp = np.zeros((T, V), dtype=F)
    if not (zero_infinity and nll == np.inf):
        with np.errstate(**_quiet):
            dlp[:Tb] = emulate_grad_stage(lp[:Tb], alpha + beta, nll, labels, blank, gs, mutant)
    return dict(alpha=alpha, beta=beta, nll=nll, dlp=dlp)


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def _absmax_finite(x):
    y = np.where(np.isfinite(x), np.abs(x), 0.0)
    return y.max(axis=1) if y.shape[1] else np.zeros(len(y))


def lattice_bound(lattice, q, reverse=False):
    """(frames,) bound of derivation (2) for every cell of a frame, from the float64 lattice and its gathered log-probs."""
    A, Q = _absmax_finite(lattice), _absmax_finite(q)
    n = len(A)
    out = np.zeros(n)
    order = range(n - 2, -1, -1) if reverse else range(1, n)
    prev = 0.0
    for t in order:
        prev = prev + E_LSE3 + U * (2.0 * (A[t] + prev) + Q[t])
        out[t] = prev
    return out


def ref_bounds(ref):
    """(alpha's, beta's) lattice_bound of a reference, computed once."""
    if "_bounds" not in ref:
        ref["_bounds"] = (lattice_bound(ref["alpha"], ref["q"]), lattice_bound(ref["beta"], ref["q"], reverse=True))
    return ref["_bounds"]


def nll_bound(ref):
    if ref["nll"] == np.inf:
        return 0.0
    return float(ref_bounds(ref)[0][-1]) + 5 * U + U * abs(ref["nll"])


def class_counts(labels, blank, V):
    k = np.bincount(np.asarray(labels, dtype=np.int64), minlength=V).astype(np.float64)
    k[blank] = len(labels) + 1
    return k


def _delta_stage(lcab, nll, lp, k):
    with np.errstate(**_quiet):
        mags = np.abs(lcab) + np.abs(lcab + nll) + np.abs(lcab + nll - lp)
        mags = np.where(np.isfinite(mags), mags, 0.0)
    return U * (mags + 2 * np.maximum(1.0, np.log(np.maximum(k, 1.0))) + (k + 8) * (4 + np.log(k + 1)) + 2)


def grad_stage(lp, ab32, nll32, labels, blank, gs):
    """Derivation (4): the float64 gradient formula on the stage's own float32 inputs, and the bound on a float32 evaluation of it.
    lp (Tb, V), ab32 (Tb, S) = fl(alpha + beta), nll32, gs the float64 value of the float32 scale.  -> (g*, bound), (Tb, V)."""
    lp, ab = np.asarray(lp, dtype=np.float64), np.asarray(ab32, dtype=np.float64)
    nll = float(nll32)
    ext = ext_labels(labels, blank)
    V = lp.shape[1]
    lcab = np.full(lp.shape, NINF)
    for c in np.unique(ext):
        lcab[:, c] = _lse_rows(ab[:, ext == c], 1)
    with np.errstate(**_quiet):
        p = np.exp(lcab + nll - lp)
        el = np.exp(lp)
        g = (el - p) * gs
        delta = _delta_stage(lcab, nll, lp, class_counts(labels, blank, V)[None, :])
        bound = abs(gs) * (p * np.expm1(delta) + 5 * U * np.maximum(el, p)) + 1e-37
    return g, bound


def composed_grad_bound(ref, lp, labels, blank, gs):
    """Derivation (5): end to end against the float64 reference.  (Tb, V); inf where the exponent's bound overflows."""
    lp = np.asarray(lp, dtype=np.float64)[:ref["post"].shape[0]]
    V = lp.shape[1]
    ba, bb = ref_bounds(ref)
    with np.errstate(**_quiet):
        lat = (ba + bb + U * (_absmax_finite(ref["ab"]) + ba + bb))[:, None] + nll_bound(ref)
        nll = ref["nll"] if np.isfinite(ref["nll"]) else 0.0
        delta = _delta_stage(ref["lcab"], nll, lp, class_counts(labels, blank, V)[None, :]) * (1 + 1e-3) + lat * (1 + 6 * U)
        p = np.where(np.isfinite(ref["post"]), ref["post"], 0.0)
        el = np.exp(lp)
        return abs(gs) * (p * np.expm1(delta) + 5 * U * np.maximum(el, p * np.exp(delta))) + 1e-37


def log_softmax_bound(x):
    """Derivation (6), forward: (rows, V) from the float64 logits."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[-1]
    lse = _lse_rows(x, -1)[..., None]
    with np.errstate(**_quiet):
        lp = x - lse
    n_add = -(-V // 64) + 6
    mag = np.where(np.isfinite(lse), np.abs(lse), 0.0) + np.where(np.isfinite(lp), np.abs(lp), 0.0)
    return U * (n_add + 3 + 2 * max(1.0, math.log(V)) + mag)


def log_softmax_bwd_bound(lp, g):
    lp, g = np.asarray(lp, dtype=np.float64), np.asarray(g, dtype=np.float64)
    V = lp.shape[-1]
    n_add = -(-V // 64) + 6
    with np.errstate(**_quiet):
        el = np.exp(lp)
        s, sa = g.sum(axis=-1, keepdims=True), np.abs(g).sum(axis=-1, keepdims=True)
        dx = g - el * s
        return U * (el * (n_add * sa + 3 * np.abs(s)) + np.abs(dx)) * (1 + 1e-3) + 1e-37


# ---------------------------------------------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------------------------------------------
def make_labels(rs, L, classes, repeat=0.25):
    """L labels from `classes`, a neighbour repeated with probability `repeat`."""
    out = []
    for j in range(L):
        if j and rs.rand() < repeat:
            out.append(out[-1])
        else:
            c = int(classes[rs.randint(len(classes))])
            while j and len(classes) > 1 and c == out[-1]:
                c = int(classes[rs.randint(len(classes))])
            out.append(c)
    return np.array(out, dtype=np.int64)


def min_frames(labels):
    return len(labels) + repeats(labels)


def state_path_min(labels):
    """The fastest walk through the lattice: label states, with the blank state between equal neighbours."""
    seq = []
    for j in range(len(labels)):
        if j and labels[j] == labels[j - 1]:
            seq.append(2 * j)
        seq.append(2 * j + 1)
    return seq if seq else [0]


def random_alignment(rs, labels, Tb, blank):
    """A valid frame-level alignment (class per frame) of `labels` over Tb >= min_frames(labels) frames."""
    seq = state_path_min(labels)
    room = Tb - len(seq)
    assert room >= 0
    L = len(labels)
    if L:                                          # optional blanks: in front, behind, between different neighbours
        gaps = [0, 2 * L] + [2 * j for j in range(1, L) if labels[j] != labels[j - 1]]
        take = [g for g in gaps if rs.rand() < 0.3][:room // 2]
        seq = sorted(seq + take)
    extra = Tb - len(seq)
    dup = rs.multinomial(extra, np.full(len(seq), 1.0 / len(seq))) if extra else np.zeros(len(seq), dtype=int)
    states = np.repeat(np.array(seq), dup + 1)
    return ext_labels(labels, blank)[states], states


def _gauss_logits(rs, T, V, std):
    return (std * rs.standard_normal((T, V))).astype(F).astype(np.float64)


def _peaked(rs, T, V, path, M):
    x = 0.5 * rs.standard_normal((T, V))
    x[np.arange(len(path)), path] += M
    return log_softmax64(x).astype(F)


REGIMES = ("gauss", "aligned8", "aligned100", "aligned1e4", "misaligned8", "misaligned100", "misaligned1e4", "uniform0", "uniformV",
           "shifted", "single_path", "one_short", "masked_classes", "blank_forbidden", "cut", "wall")
REDUCED = ("misaligned100", "uniformV", "single_path", "cut", "wall", "gauss")
_PEAK = {"8": 8.0, "100": 100.0, "1e4": 1e4}


def make_utterance(name, seed, T, V, Lcap, blank, L=None, slack=None):
    """One utterance of a regime: dict name, lp (T, V) float32, labels, in_len, and what the regime promises (feasible, path, uniform_c,
    cut = (frame, state), M).  L <= Lcap is drawn unless given, in_len <= T is drawn or (slack) min_frames + slack; every length is valid."""
    rs = np.random.RandomState((seed * 1000003 + REGIMES.index(name) * 7919 + 17 * blank + 1) % (2 ** 31))
    other = [c for c in range(V) if c != blank]
    rs.shuffle(other)
    reserved, classes = other[:4], other[4:]                    # four non-blank classes kept out of the label strings
    if L is None:
        L = Lcap if name in ("gauss", "single_path", "one_short", "misaligned100") else int(rs.randint(max(Lcap // 2, 1), Lcap + 1))
    labels = make_labels(rs, L, classes)
    u = dict(name=name, labels=labels, feasible=True, blank=blank)
    need = min_frames(labels)
    assert need <= T, (name, need, T)
    if slack is not None:
        in_len = min(T, need + slack)
    else:
        in_len = T if name in ("gauss", "misaligned100") else int(rs.randint(min(need + 3 + (T - need) // 2, T), T + 1))
    Tb = in_len
    if name == "gauss":
        lp = log_softmax64(_gauss_logits(rs, T, V, 2.0)).astype(F)
    elif name.startswith("aligned") or name.startswith("misaligned"):
        M = _PEAK[name[name.index("d") + 1:]]
        src = labels
        if name.startswith("mis"):
            src = make_labels(rs, L, classes)
            while L and np.array_equal(src, labels):
                src = make_labels(rs, L, classes)
            Tb = max(Tb, min_frames(src))
            assert Tb <= T
        path, _ = random_alignment(rs, src, Tb, blank)
        lp = _peaked(rs, T, V, path, M)
        u.update(M=M)
    elif name in ("uniform0", "uniformV"):
        c = F(0.0) if name == "uniform0" else F(-math.log(V))
        lp = np.full((T, V), c, dtype=F)
        u.update(uniform_c=float(c))
    elif name == "shifted":
        lp = (log_softmax64(_gauss_logits(rs, T, V, 2.0)) + rs.uniform(-8, 8, size=(T, 1))).astype(F)
    elif name in ("single_path", "one_short"):
        lp = (rs.randint(-511, 0, size=(T, V)) / 64.0).astype(F)
        Tb = need if name == "single_path" else need - 1
        u.update(path=np.array(state_path_min(labels)), feasible=name == "single_path")
        assert Tb >= 1
    elif name == "masked_classes":
        x = _gauss_logits(rs, T, V, 2.0)
        x[:, reserved[:3]] = NINF
        lp = log_softmax64(x).astype(F)
        u.update(masked=reserved[:3])
    elif name == "blank_forbidden":
        path, _ = random_alignment(rs, labels, Tb, blank)
        x = _gauss_logits(rs, T, V, 2.0)
        free = np.flatnonzero(path != blank)
        hit = rs.choice(free, size=min(len(free), Tb // 3), replace=False)
        x[hit, blank] = NINF
        lp = log_softmax64(x).astype(F)
        u.update(forbidden=np.sort(hit))
    elif name == "cut":
        j = L // 2
        labels[j] = reserved[3]                                   # occurs once: the class is in no other position
        Tb = max(Tb, min_frames(labels) + 2)
        assert Tb <= T
        _, states = random_alignment(rs, labels, Tb, blank)
        tc = int(np.flatnonzero(states == 2 * j + 1)[0])
        x = _gauss_logits(rs, T, V, 2.0)
        x[tc, :] = NINF
        x[tc, reserved[3]] = 0.0
        lp = log_softmax64(x).astype(F)
        u.update(cut=(tc, 2 * j + 1))
    elif name == "wall":
        x = _gauss_logits(rs, T, V, 2.0)
        tw = Tb // 2
        x[tw, np.unique(ext_labels(labels, blank))] = NINF
        lp = log_softmax64(x).astype(F)
        u.update(feasible=False, wall=tw)
    else:
        raise KeyError(name)
    u.update(lp=lp, in_len=int(Tb))
    return u


# (Lmax, T, V, regimes): the smallest label rows that reach each launch of plan_ctc_lattice
SHAPES = ((5, 24, 20, REGIMES), (40, 100, 20, REGIMES), (127, 280, 20, REGIMES), (128, 280, 62, REGIMES), (300, 640, 62, REGIMES),
          (600, 1250, 62, REDUCED), (1100, 2250, 62, REDUCED))
PLANS = {5: (1, 1, 1), 40: (1, 2, 1), 127: (1, 4, 1), 128: (0, 5, 2), 300: (0, 10, 4), 600: (0, 19, 8), 1100: (0, 35, 16)}   # skewed, waves, ns
_cache = {}


def batch(Lmax, blank=0):
    """The batch of a shape: dict T, B, V, Lmax, lp (T, B, V) float32, targets (B, Lmax) int64 (padded with a valid class), in_len, tgt_len,
    utts.  Built once per (Lmax, blank) and shared; callers must not write to it."""
    key = (Lmax, blank)
    if key in _cache:
        return _cache[key]
    _, T, V, names = [s for s in SHAPES if s[0] == Lmax][0]
    utts = []
    for name in names:
        kw = {}
        if names is REDUCED:                                      # the two largest rows: two utterances at full size, the rest smaller
            if name == "uniformV":
                kw = dict(L=Lmax // 3, slack=24)                  # a narrow band keeps the integer counter cheap
            elif name in ("gauss", "cut", "wall"):
                kw = dict(L=Lmax // 2)
        utts.append(make_utterance(name, Lmax, T, V, Lmax, blank, **kw))
    B = len(utts)
    pad = (blank + 1) % V
    tg = np.full((B, Lmax), pad, dtype=np.int64)
    for i, u in enumerate(utts):
        tg[i, :len(u["labels"])] = u["labels"]
    out = dict(T=T, B=B, V=V, Lmax=Lmax, blank=blank, lp=np.ascontiguousarray(np.stack([u["lp"] for u in utts], axis=1)), targets=tg,
               in_len=np.array([u["in_len"] for u in utts], dtype=np.int64),
               tgt_len=np.array([len(u["labels"]) for u in utts], dtype=np.int64), utts=utts)
    out["lp"].setflags(write=False)
    _cache[key] = out
    return out


_ref_cache = {}


def batch_reference(Lmax, blank=0):
    """reference() of every utterance of batch(Lmax, blank), computed once."""
    key = (Lmax, blank)
    if key not in _ref_cache:
        b = batch(Lmax, blank)
        _ref_cache[key] = [reference(u["lp"], u["labels"], u["in_len"], blank) for u in b["utts"]]
    return _ref_cache[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# the checks both test files apply to one utterance's result (the emulation's on the CPU, a kernel form's on the GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def check_utterance(u, ref, got, gs=1.0, zero_infinity=False):
    """got: alpha, beta (in_len, S) float32 (beta may be None), ab (in_len, S) float32 = fl(alpha + beta) (None: formed here), nll float32,
    dlp (T, V) float32 or None -- the gradient for the float64 scale gs.  Returns (violations, ratios): the names of the claims the result
    breaks (empty for a correct float32 implementation) and the worst error / bound ratio per quantity."""
    bad, ratio = [], {}
    Tb = int(u["in_len"])
    lp = np.asarray(u["lp"], dtype=np.float64)

    def lattice(name, reverse):
        x, r = got.get(name), ref[name]
        if x is None:
            return
        x = np.asarray(x)
        if x.shape != r.shape or not np.array_equal(np.isneginf(x), np.isneginf(r)) or not np.isfinite(x[np.isfinite(r)]).all():
            bad.append(name + ":-inf pattern")
            return
        b = ref_bounds(ref)[1 if reverse else 0][:, None] + np.zeros_like(r)
        fin = np.isfinite(r)
        err = np.abs(x.astype(np.float64)[fin] - r[fin])
        ok = err <= b[fin]
        pos = b[fin] > 0
        ratio[name] = float((err[pos] / b[fin][pos]).max()) if pos.any() else 0.0
        if not ok.all():
            bad.append(name + ":bound")
        if "path" in u and u["feasible"]:
            t = np.arange(Tb)
            if not np.array_equal(x[t, u["path"]], r[t, u["path"]].astype(F)):
                bad.append(name + ":single path bits")

    lattice("alpha", False)
    lattice("beta", True)
    nll = float(got["nll"])
    if (nll == np.inf) != (ref["nll"] == np.inf) or np.isnan(nll):
        bad.append("nll:inf pattern")
    elif np.isfinite(nll):
        nb = nll_bound(ref)
        ratio["nll"] = abs(nll - ref["nll"]) / nb
        if ratio["nll"] > 1:
            bad.append("nll:bound")
        if "path" in u and F(ref["nll"]) != F(nll):
            bad.append("nll:single path bits")
    if got.get("dlp") is not None:
        dlp = np.asarray(got["dlp"])
        want = ref_dlp(ref, lp, gs, zero_infinity)
        if not np.array_equal(np.isnan(dlp), np.isnan(want)) or np.isinf(dlp).any():
            bad.append("dlp:NaN mask")
        if dlp[Tb:].any() or np.signbit(dlp[Tb:]).any():
            bad.append("dlp:rows past in_len")
        if zero_infinity and ref["nll"] == np.inf:
            if dlp.any():
                bad.append("dlp:zero_infinity")
        elif got.get("ab") is not None or got.get("beta") is not None:
            ab = got["ab"] if got.get("ab") is not None else np.asarray(got["alpha"], dtype=F) + np.asarray(got["beta"], dtype=F)
            g64, gb = grad_stage(lp[:Tb], ab, got["nll"], u["labels"], u["blank"], gs)
            fin = np.isfinite(g64) & np.isfinite(dlp[:Tb])
            err = np.abs(dlp[:Tb].astype(np.float64)[fin] - g64[fin])
            ratio["grad_stage"] = float((err / gb[fin]).max()) if fin.any() else 0.0
            if not np.array_equal(np.isnan(g64), np.isnan(dlp[:Tb])):
                bad.append("dlp:stage NaN mask")
            if ratio["grad_stage"] > 1:
                bad.append("dlp:stage bound")
        fin = np.isfinite(want) & np.isfinite(dlp)
        if fin[:Tb].any():
            err = np.abs(dlp.astype(np.float64) - want)[:Tb]
            ratio["dlp_end_to_end"] = float(err[fin[:Tb]].max())
            cb = composed_grad_bound(ref, lp, u["labels"], u["blank"], gs)
            with np.errstate(**_quiet):
                if not (err[fin[:Tb]] <= cb[fin[:Tb]]).all():
                    bad.append("dlp:composed bound")
    return bad, ratio
