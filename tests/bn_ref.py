"""float64 restatement of BatchNorm, a replay of norm.hip's stated arithmetic, and derived error bounds  --  TEST INFRASTRUCTURE ONLY
(used by test_bn_regimes*.py and test_length_mask.py).

Everything works on x viewed as (outer, C, inner) with an optional validity mask of the same shape (the length-aware entry points; the rule
of include/ctcn.h is `_valid`).  Statistics run per channel over the n valid elements.

1. The RESTATEMENT (`train_fwd`, `train_bwd`, `running_update`, `eval_fwd`): plain numpy float64, two-pass variance mean((x - mean)^2),
   never E[x^2] - mean^2.  tests/test_bn_regimes_host.py holds it to torch.nn.BatchNorm1d / 2d in float64 to 1e-12.
   The guards are those of bn_finalize_stats_kernel: n = 0 gives mean 0, var 0; n <= 1 updates running_var with the biased variance.

2. `kernel_model`: what norm.hip says it computes, replayed in numpy float32 / float64 --
     s, ss        float64 sums of x and x * x (the product of two float32 is exact in float64)
     mean, var    s / n and max(ss / n - mean^2, 0) in float64; save_mean = fl32(mean), save_rstd = fl32(1 / sqrt(var + eps))
     y            bn_value:     fma(fl32(fl32(x - m) * rs), g, b)
     s0, s1       float64 sums of dy' and dy' * xhat with xhat = fl32(fl32(x - m) * rs); dbeta = fl32(s0), dgamma = fl32(s1)
     dx           bn_dx_value:  fl32(fl32(ga * rs) * fma(-xh, fl32(s1 * inv_n), fma(-s0, inv_n, g))), s0, s1, inv_n rounded to float32
     eval         rs = 1 / sqrtf(rv + eps): three float32 roundings
   numpy has no fma: the fused operations are formed in float64 and rounded once (a * b is exact there; the sum is rounded to 53 bits and
   then to 24, which differs from the single rounding only where the 53-bit sum falls on a float32 midpoint: ~2^-29 of all elements).
   The per-element expressions are also a BIT contract (norm.hip: "ONE rounding sequence" for every apply / dx kernel, fused or not):
   `model_value` / `model_dx` from the kernel's own save_mean, save_rstd, dbeta, dgamma must give the kernel's y and dx bit for bit --
   REPLAY_MISMATCH allows the emulation's double rounding and nothing else; a reordered expression moves the bits of a third of the
   elements while staying inside any error bound.  The model is NOT the reference.  It separates a wrong
   bound from a wrong kernel: if the model stays inside `bounds` on an input and the kernel does not, the kernel is wrong.

3. `bounds`: per-element / per-channel bounds on |device value - float64 value|, by running error analysis of that arithmetic.  Nothing
   is fitted to a kernel's output.  u = 2^-24 (a float32 rounding to nearest: relative u), w = 2^-53 (float64), n = valid elements of the
   channel.  A float64 sum of n terms, in ANY order, is off by at most n w sum|terms| (n - 1 additions, each rounding a partial sum that
   is at most sum|terms|): the chain length n is an upper bound no summation order exceeds.
     mean64       |s_dev / n - mean| <= (n + 1) w mean|x|                                                   =: e_mu
     save_mean    e_m = u |mean| + e_mu                           (+ 2^-150: the float32 subnormal spacing; on every float32 result below)
     var          ss / n is off by (n + 1) w mean(x^2); mean_dev^2 by 2 |mean| e_mu + w mean^2; the subtraction rounds once:
                  e_var = (n + 1) w mean(x^2) + 2 |mean| e_mu + 2 w mean(x^2)
                  For a centred channel that is n w mean(x^2); for one with |mean| >> spread 3 n w mean^2 -- the cancellation of
                  E[x^2] - mean^2, which is all that covers `twopoint`.  The device clamps var at 0.
     save_rstd    the interval [1 / sqrt(var + e_var + eps), 1 / sqrt(max(var - e_var, 0) + eps)] (no linearisation: e_var may exceed
                  var + eps), widened by (u + 4 w) rstd for sqrt, division and the float32 rounding                    =: e_rs
     running      rm: mom e_mu + u |rm'| ;  rv: mom e_var n / (n - 1) + u |rv'|   (one float32 rounding on top, + 4 w of the float64 expression)
     y            d = fl32(x - m):  |d - (x - mean)| <= e_m + r_sub, r_sub = u |x - m|, and r_sub = 0 where the subtraction is exact for
                  every m within e_m of the mean: Sterbenz (m / 2 <= x <= 2 m) or x = 0
                  t = fl32(d rs):   e_t = e_d (rstd + e_rs) + |x - mean| e_rs, + u |t|               (t is also the xhat of the backward pass)
                  y = fma(t, g, b): e_y = |g| e_t + u (|y| + |g| e_t)
                  i.e. the mean error times |gamma| rstd, the rstd error times |gamma (x - mean)|, and three roundings.  ReLU is 1-Lipschitz.
     dbeta        e_s0 = n w sum|dy'| ; + u |s0| for the float32 store; beta_acc: + u |s0 + base| for the accumulate
     dgamma       sum dy' t with t = (x - mean + delta)(rstd + eps_rs)(1 + rho): xhat's shift delta = mean - m and its scale error are COMMON
                  to the channel and meet the signed sums, only the roundings rho (the subtraction unless exact, the product) meet sum|dy'|:
                  e_s1 = |s1| e_rs / rstd + (rstd + e_rs) e_m |s0| + sum|dy'| (|x - mean| + e_m)(rstd + e_rs) rho + n w sum|dy'| (|xhat| + e_t);
                  then as dbeta.  (sum|dy'| e_t would also hold, and grows as n where this grows as sqrt(n) + 2 u n E|dy' xhat|.)
     constants    a channel whose valid elements all hold one value a, with n a and n a^2 within 53 bits: every partial sum of both float64
                  sums is representable, so s / n = a and ss / n - a^2 = 0 exactly in any order: e_mu = e_m = e_var = 0
     dx           A = fma(-s0, inv_n, g), B = fl32(s1 inv_n), Cc = fma(-xh, B, A), G = fl32(ga rs), dx = fl32(G Cc): each operand carries its
                  bound (s0, s1: e_s + u |s|; inv_n: u / n), products propagate as |a| e_b + |b| e_a + e_a e_b, each result adds u |result|
     eval         rs = 1 / sqrtf(rv + eps): 3 u relative (sum, square root and division are correctly rounded: 2.5 u to first order);
                  m = running_mean is exact; then as y
   What the bounds say where they are wide (test_bn_regimes_host.py enforces that they are not, elsewhere):
     offset_tight, offset3, offset5   e_y ~ |gamma| rstd ulp(mean) / 2: save_mean is a float32.  mean 300, std 0.03: 1.5e-5 * 33 = 5e-4.
     const, const_neg                 would carry the same term (0.8 for -3e4 * 316) but for the rule for constants above; the GPU test also
                                      asserts the exact values there
     twopoint                         the two values are one ulp apart and fl32(mean) is one of them: xhat is off by as much as it is large
                                      (0.08), and e_var = 3 n w 4096^2 passes eps at n = 2e3: nothing can be asked of y but its order of
                                      magnitude, and of rstd but its interval

4. The REGIMES (one per channel: channel c takes REGIMES[c % 14], dy regime DY_REGIMES[(c + c // 14 + shift) % 4]), the CASES the GPU test
   runs, and the eval-only statistics grid, so that the host tests (which check the regimes' stated conditions and the non-vacuity of the
   bounds) and the GPU tests draw identical tensors.
"""
import numpy as np

U = 2.0 ** -24
W = 2.0 ** -53
TINY = 2.0 ** -150
EPS = float(np.float32(1e-5))         # the float32 values the ABI receives
MOM = float(np.float32(0.1))


def _valid(layout, lens, outer, C, inner, frame):
    """bool (outer, C, inner): the validity rule of include/ctcn.h."""
    lens = np.asarray(lens)
    if layout == "rows":
        r = np.arange(outer)
        v = (r // len(lens)) < lens[r % len(lens)]
        return np.broadcast_to(v[:, None, None], (outer, C, 1))
    v = (np.arange(inner)[None, :] // frame) < lens[:, None]
    return np.broadcast_to(v[:, None, :], (outer, C, inner))


def _b(a):
    return np.asarray(a)[None, :, None]


def _all(x, valid):
    return np.ones(x.shape, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)


def _msum(a, v):
    return np.where(v, a, 0.0).sum(axis=(0, 2))


def _count(v):
    return float(v[:, 0, :].sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def train_fwd(x, gamma, beta, valid=None, eps=EPS):
    """{n, mean, var (biased), rstd, xhat, y, y_relu}; y, y_relu are 0 at invalid elements."""
    x, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta))
    v = _all(x, valid)
    n = _count(v)
    C = x.shape[1]
    if n > 0:
        mean = _msum(x, v) / n
        var = _msum((x - _b(mean)) ** 2, v) / n
    else:
        mean, var = np.zeros(C), np.zeros(C)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = np.where(v, (np.where(v, x, 0.0) - _b(mean)) * _b(rstd), 0.0)
    y = np.where(v, xhat * _b(gamma) + _b(beta), 0.0)
    return {"n": n, "mean": mean, "var": var, "rstd": rstd, "xhat": xhat, "y": y, "y_relu": np.maximum(y, 0.0)}


def train_bwd(fwd, gamma, g, valid=None):
    """g = dy' (dy with the ReLU mask applied, any value at invalid elements).  {dx, dgamma, dbeta, s0, s1}."""
    gamma = np.asarray(gamma, dtype=np.float64)
    v = _all(fwd["xhat"], valid)
    g = np.where(v, np.asarray(g, dtype=np.float64), 0.0)
    n, xh = fwd["n"], fwd["xhat"]
    s0, s1 = g.sum(axis=(0, 2)), (g * xh).sum(axis=(0, 2))
    inv = 1.0 / n if n > 0 else 0.0
    dx = np.where(v, _b(gamma * fwd["rstd"]) * (g - _b(s0) * inv - xh * _b(s1) * inv), 0.0)
    return {"dx": dx, "dgamma": s1, "dbeta": s0, "s0": s0, "s1": s1, "g": g}


def running_update(rm0, rv0, mean, var, n, mom=MOM):
    rm0, rv0 = np.asarray(rm0, dtype=np.float64), np.asarray(rv0, dtype=np.float64)
    unbiased = var * n / (n - 1.0) if n > 1 else var
    return (1.0 - mom) * rm0 + mom * mean, (1.0 - mom) * rv0 + mom * unbiased


def eval_fwd(x, gamma, beta, rm, rv, valid=None, eps=EPS, relu=False):
    x, gamma, beta, rm, rv = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta, rm, rv))
    v = _all(x, valid)
    y = (np.where(v, x, 0.0) - _b(rm)) * _b(1.0 / np.sqrt(rv + eps)) * _b(gamma) + _b(beta)
    return np.where(v, np.maximum(y, 0.0) if relu else y, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the kernel's stated arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def _r(a):
    """one rounding to float32, returned as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def model_value(x, m, rs, g, b):
    """bn_value; all arguments float32 values held in float64"""
    return _r(_r(_r(x - m) * rs) * g + b)


def kernel_model(x, gamma, beta, dy, valid=None, rm0=None, rv0=None, relu=False, eps=EPS, mom=MOM, base=None, mask=None):
    """Forward, backward (beta_acc = 1 where `base` = (dgamma0, dbeta0) is given) and running statistics as norm.hip states them.
    mask: the ReLU mask to use in the backward pass (default: the model's own y > 0).  float64 arrays holding float32 values."""
    x, gamma, beta, dy = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta, dy))
    v = _all(x, valid)
    n, C = _count(v), x.shape[1]
    xz = np.where(v, x, 0.0)
    if n > 0:
        mean = _msum(xz, v) / n
        var = np.maximum(_msum(xz * xz, v) / n - mean * mean, 0.0)
    else:
        mean, var = np.zeros(C), np.zeros(C)
    m, rs = _r(mean), _r(1.0 / np.sqrt(var + eps))
    out = {"save_mean": m, "save_rstd": rs}
    if rm0 is not None:
        unbiased = var * n / (n - 1.0) if n > 1 else var
        out["running_mean"] = _r((1.0 - mom) * np.asarray(rm0, dtype=np.float64) + mom * mean)
        out["running_var"] = _r((1.0 - mom) * np.asarray(rv0, dtype=np.float64) + mom * unbiased)
    xh = _r(_r(xz - _b(m)) * _b(rs))
    y = _r(xh * _b(gamma) + _b(beta))
    if relu:
        keep = (y > 0) if mask is None else mask
        y = np.maximum(y, 0.0)
    else:
        keep = np.ones_like(v)
    out["y"] = np.where(v, y, 0.0)
    g = np.where(v & keep, dy, 0.0)
    s0_64, s1_64 = g.sum(axis=(0, 2)), (g * np.where(v, xh, 0.0)).sum(axis=(0, 2))
    s0, s1 = _r(s0_64), _r(s1_64)
    out["dbeta"], out["dgamma"] = s0, s1
    if base is not None:
        out["dgamma"], out["dbeta"] = _r(s1 + np.asarray(base[0], dtype=np.float64)), _r(s0 + np.asarray(base[1], dtype=np.float64))
    out["dx"] = model_dx(xz, g, gamma, m, rs, s0, s1, n, v)
    return out


def model_dx(xz, g, gamma, m, rs, s0, s1, n, v):
    """bn_dx_value on float32 values held in float64: g = dy' (0 where masked), m / rs / s0 / s1 the float32 per-channel values"""
    inv_n = float(_r(1.0 / n)) if n > 0 else 0.0
    xh = _r(_r(xz - _b(m)) * _b(rs))
    a = _r(g - _b(s0) * inv_n)
    bb = _r(s1 * inv_n)
    cc = _r(a - xh * _b(bb))
    return np.where(v, _r(_b(_r(gamma * rs)) * cc), 0.0)


def model_eval(x, gamma, beta, rm, rv, valid=None, relu=False, eps=EPS):
    x, gamma, beta, rm, rv = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta, rm, rv))
    v = _all(x, valid)
    rs = _r(1.0 / _r(np.sqrt(_r(rv + eps))))
    y = model_value(np.where(v, x, 0.0), _b(rm), _b(rs), _b(gamma), _b(beta))
    return np.where(v, np.maximum(y, 0.0) if relu else y, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the bounds (module docstring, point 3)
# ---------------------------------------------------------------------------------------------------------------------------------
def _rnd(v, e):
    """the bound of a float32 result of float64 value v whose exact-arithmetic counterpart is within e"""
    return e + U * (np.abs(v) + e) + TINY


def _sub_exact(x, m_lo, m_hi):
    """x - m is exact in float32 for every m in [m_lo, m_hi]: Sterbenz, or x = 0"""
    same = (np.sign(x) == np.sign(m_lo)) & (np.sign(x) == np.sign(m_hi)) & (x != 0)
    big, small = np.maximum(np.abs(m_lo), np.abs(m_hi)), np.minimum(np.abs(m_lo), np.abs(m_hi))
    return (x == 0) | (same & (np.abs(x) >= big / 2.0) & (np.abs(x) <= 2.0 * small))


def _const_exact(xz, v, n):
    """bool per channel: all valid elements hold one value a, and n a and n a^2 need at most 53 bits -- then every partial sum of the
    float64 sums of x and x * x is exact in any order, s / n = a, ss / n - a^2 = 0"""
    C = xz.shape[1]
    res = np.zeros(C, dtype=bool)
    if n <= 0:
        return res
    for c in range(C):
        vals = xz[:, c, :][v[:, c, :]]
        a = float(vals[0])
        if np.all(vals == a):
            num = abs(int(np.frexp(a)[0] * 2 ** 24)) if a != 0 else 0          # 24-bit significand of a float32 as an integer
            num = num // (num & -num) if num else 0                             # its odd part
            res[c] = (num * num).bit_length() + int(n).bit_length() <= 53
    return res


def _apply_bounds(x, v, centre, e_m, scale, e_rs, gamma, beta):
    """(e_t, e_y) of t = fl32(fl32(x - m) rs) and y = fma(t, g, b) for m within e_m of centre and rs within e_rs of scale (per channel)"""
    xz = np.where(v, x, 0.0)
    d = xz - _b(centre)
    exact = _sub_exact(xz, _b(centre - e_m), _b(centre + e_m))
    e_d = _b(e_m) + np.where(exact, 0.0, U * (np.abs(d) + _b(e_m)))
    t = d * _b(scale)
    e_t = _rnd(t, e_d * _b(scale + e_rs) + np.abs(d) * _b(e_rs))
    y = t * _b(gamma) + _b(beta)
    e_y = _rnd(y, np.abs(_b(gamma)) * e_t)
    return np.where(v, e_t, 0.0), np.where(v, e_y, 0.0)


def bounds(x, gamma, beta, fwd, bwd=None, valid=None, rm0=None, rv0=None, base=None, eps=EPS, mom=MOM):
    """fwd = train_fwd(...), bwd = train_bwd(...) or None.  Returns {save_mean, save_rstd, running_mean, running_var, y, dgamma, dbeta, dx}:
    bounds on |device - float64 restatement|, per channel or per element."""
    x, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta))
    v = _all(x, valid)
    n, mean, var, rstd = fwd["n"], fwd["mean"], fwd["var"], fwd["rstd"]
    xz = np.where(v, x, 0.0)
    if n > 0:
        m1, m2 = _msum(np.abs(xz), v) / n, _msum(xz * xz, v) / n
    else:
        m1, m2 = np.zeros_like(mean), np.zeros_like(mean)
    e_mu = (n + 1) * W * m1
    e_m = U * np.abs(mean) + e_mu + TINY
    e_var = (n + 1) * W * m2 + 2.0 * np.abs(mean) * e_mu + 2.0 * W * m2
    for c in np.flatnonzero(_const_exact(xz, v, n)):          # every partial sum is representable: mean = the value, var = 0, exactly
        e_mu[c] = e_m[c] = e_var[c] = 0.0
    lo, hi = 1.0 / np.sqrt(var + e_var + eps), 1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps)
    e_rs = np.maximum(hi - rstd, rstd - lo) + (U + 4 * W) * hi
    out = {"save_mean": e_m, "save_rstd": e_rs, "e_var": e_var}
    if rm0 is not None:
        rm_ref, rv_ref = running_update(rm0, rv0, mean, var, n, mom)
        ub = n / (n - 1.0) if n > 1 else 1.0
        out["running_mean"] = mom * e_mu + (U + 4 * W) * (np.abs(rm_ref) + mom * e_mu) + TINY
        out["running_var"] = mom * e_var * ub + (U + 4 * W) * (np.abs(rv_ref) + mom * e_var * ub) + TINY
    e_t, e_y = _apply_bounds(x, v, mean, e_m, rstd, e_rs, gamma, beta)
    out["y"], out["xhat"] = e_y, e_t
    if bwd is None:
        return out
    g, xh = np.abs(bwd["g"]), np.abs(fwd["xhat"])
    s0, s1 = bwd["s0"], bwd["s1"]
    e_s0 = n * W * g.sum(axis=(0, 2))
    # sum g t with t = (x - mean + delta)(rstd + eps_rs)(1 + rho): the shift delta = mean - m and the scale error are COMMON to the channel
    # and meet the signed sums s0 and s1; only the roundings rho (subtraction unless exact, product) meet sum|g|
    d = np.abs(xz - _b(mean))
    exact = _sub_exact(xz, _b(mean - e_m), _b(mean + e_m))
    rho = np.where(exact, 0.0, U) + U + U * U
    e_s1 = (np.abs(s1) * e_rs / rstd + (rstd + e_rs) * e_m * np.abs(s0) + (g * ((d + _b(e_m)) * _b(rstd + e_rs) * rho + TINY)).sum(axis=(0, 2))
            + n * W * (g * (xh + e_t)).sum(axis=(0, 2)))
    e_s0f, e_s1f = _rnd(s0, e_s0), _rnd(s1, e_s1)
    out["dbeta"], out["dgamma"] = e_s0f, e_s1f
    if base is not None:
        out["dgamma"] = _rnd(s1 + np.asarray(base[0], dtype=np.float64), e_s1f)
        out["dbeta"] = _rnd(s0 + np.asarray(base[1], dtype=np.float64), e_s0f)
    inv = 1.0 / n if n > 0 else 0.0
    e_inv = U * inv
    mul = lambda a, ea, b, eb: np.abs(a) * eb + np.abs(b) * ea + ea * eb
    a_ref = bwd["g"] - _b(s0) * inv
    e_a = _rnd(a_ref, _b(mul(s0, e_s0f, inv, e_inv)))
    b_ref = s1 * inv
    e_b = _rnd(b_ref, mul(s1, e_s1f, inv, e_inv))
    c_ref = a_ref - fwd["xhat"] * _b(b_ref)
    e_c = _rnd(c_ref, e_a + mul(fwd["xhat"], e_t, _b(b_ref), _b(e_b)))
    gr = gamma * rstd
    e_g = _rnd(gr, np.abs(gamma) * e_rs)
    out["dx"] = np.where(v, _rnd(_b(gr) * c_ref, mul(_b(gr), _b(e_g), c_ref, e_c)), 0.0)
    return out


def eval_bounds(x, gamma, beta, rm, rv, valid=None, eps=EPS):
    x, gamma, beta, rm, rv = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta, rm, rv))
    rs = 1.0 / np.sqrt(rv + eps)
    return _apply_bounds(x, _all(x, valid), rm, np.zeros_like(rm), rs, 3.0 * U * rs * (1.0 + 3.0 * U), gamma, beta)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. regimes and cases
# ---------------------------------------------------------------------------------------------------------------------------------
REGIMES = ("gauss", "logmel", "offset3", "offset5", "offset_tight", "const0", "const", "const_neg", "sparse", "spike", "tiny", "huge", "vast",
           "twopoint")
CONST_VALUE = {"const0": 0.0, "const": 7.25, "const_neg": -3e4}
DY_REGIMES = ("gauss", "common", "small", "zero")
TWOPOINT = (np.float32(4096.0), np.nextafter(np.float32(4096.0), np.float32(np.inf)))


def regime_of(c):
    return REGIMES[c % len(REGIMES)]


def dy_regime_of(c, shift=0):
    return DY_REGIMES[(c + c // len(REGIMES) + shift) % len(DY_REGIMES)]


def regime_data(name, rs, valid2):
    """float32 (outer, inner) of one channel; valid2: bool (outer, inner) -- `spike` puts its one element on a valid position"""
    shape = valid2.shape
    z = rs.standard_normal(shape)
    if name == "gauss":
        a = 2.0 * z + 0.5
    elif name == "logmel":
        a = 15.0 + 3.0 * z
    elif name == "offset3":
        a = 1e3 + z
    elif name == "offset5":
        a = 1e5 + 30.0 * z
    elif name == "offset_tight":
        a = 300.0 + 0.03 * z
    elif name in CONST_VALUE:
        a = np.full(shape, CONST_VALUE[name])
    elif name == "sparse":
        a = np.where(rs.random_sample(shape) < 0.98, 0.0, np.abs(z) * 5.0)
    elif name == "spike":
        a = np.zeros(shape)
        idx = np.flatnonzero(valid2.ravel())
        if idx.size:
            a.ravel()[idx[rs.randint(idx.size)]] = 1e3
    elif name == "tiny":
        a = 1e-6 * z
    elif name == "huge":
        a = 1e6 * z
    elif name == "vast":
        a = 1e15 * z
    elif name == "twopoint":
        a = np.where(rs.random_sample(shape) < 0.5, TWOPOINT[0], TWOPOINT[1]).astype(np.float64)
    else:
        raise ValueError(name)
    return a.astype(np.float32)


def dy_data(name, rs, shape):
    z = rs.standard_normal(shape)
    a = {"gauss": z, "common": 1.0 + 1e-3 * z, "small": 1e-6 * z, "zero": np.zeros(shape)}[name]
    return a.astype(np.float32)


# name: layout, (outer, C, inner), storage offset of x in floats, option bn_rows4 -- the launch branch reached (test_bn_regimes.py)
CASES = {
    "rows_27x14": ("rows", (27, 14, 1), 0, 1),
    "rows_200x28": ("rows", (200, 28, 1), 0, 1),
    "rows_1500x84_off1": ("rows", (1500, 84, 1), 1, 1),
    "rows_400x84_dword": ("rows", (400, 84, 1), 0, 0),
    "nchw_3x14x200": ("nchw", (3, 14, 200), 0, 1),
    "nchw_2x14x33": ("nchw", (2, 14, 33), 0, 1),
    "nchw_3x14x28000": ("nchw", (3, 14, 28000), 0, 1),
    "nchw_200x28x37": ("nchw", (200, 28, 37), 0, 1),
    "rows_400x28_sync": ("rows", (400, 28, 1), 0, 1),
}
SYNC_CASE, SYNC_SHARDS, SYNC_SHIFT = "rows_400x28_sync", (130, 270), (-50.0, 50.0)
# name: (case, lens, batch, frame).  Every set but the guards holds a full-length, a one-frame and a zero-length utterance (the NCHW case
# of two planes: in two sets)
MASKED_CASES = {
    "rows_27x14": ("rows_27x14", [9, 1, 0], 3, 1),
    "rows_200x28": ("rows_200x28", [50, 1, 0, 33], 4, 1),
    "nchw_3x14x200": ("nchw_3x14x200", [25, 1, 0], 3, 8),
    "nchw_2x14x33_one": ("nchw_2x14x33", [11, 1], 2, 3),
    "nchw_2x14x33_zero": ("nchw_2x14x33", [0, 11], 2, 3),
    # the guards of bn_finalize_stats_kernel
    "rows_27x14_n1": ("rows_27x14", [0, 1, 0], 3, 1),
    "nchw_2x14x33_n1": ("nchw_2x14x33", [0, 1], 2, 1),
    "rows_27x14_n0": ("rows_27x14", [0, 0, 0], 3, 1),
    "nchw_2x14x33_n0": ("nchw_2x14x33", [0, 0], 2, 3),
}
DROPOUT_CASES = ("rows_200x28", "nchw_3x14x200")
EVAL_VARS = (0.0, 1e-12, 1e-5, 1.0, 1e8)
EVAL_MEANS = (0.0, 15.0, -15.0, 1e5, -1e5)

_cache = {}


def case_valid(name):
    """(case name, bool (outer, C, inner)) of a MASKED_CASES entry"""
    case, lens, batch, frame = MASKED_CASES[name]
    layout, (outer, C, inner), _, _ = CASES[case]
    return case, _valid(layout, lens, outer, C, inner, frame).copy()


def make_case(name, masked=None):
    """The tensors of a CASES entry (float32; computed once per process, shared, read-only): x, dy, gamma, beta, rm0, rv0, base_g, base_b,
    eval_rm, eval_rv, regimes, dy_regimes.  masked: a MASKED_CASES name -- `valid` is added and `spike` lands on a valid element."""
    key = (name, masked)
    if key in _cache:
        return _cache[key]
    layout, (outer, C, inner), _, _ = CASES[name]
    idx = sorted(CASES).index(name)
    rs = np.random.RandomState(7000 + 97 * idx + (0 if masked is None else 1 + sorted(MASKED_CASES).index(masked)))
    valid = np.ones((outer, C, inner), dtype=bool) if masked is None else case_valid(masked)[1]
    x, dy = np.empty((outer, C, inner), dtype=np.float32), np.empty((outer, C, inner), dtype=np.float32)
    for c in range(C):
        x[:, c, :] = regime_data(regime_of(c), rs, valid[:, c, :])
        dy[:, c, :] = dy_data(dy_regime_of(c, idx), rs, (outer, inner))
    if name == SYNC_CASE:          # the two shards differ in distribution: the global variance is mostly between-shard
        for c in range(C):
            if regime_of(c) in ("gauss", "logmel"):
                x[:SYNC_SHARDS[0], c] += np.float32(SYNC_SHIFT[0])
                x[SYNC_SHARDS[0]:, c] += np.float32(SYNC_SHIFT[1])
    sign = lambda: np.where(rs.random_sample(C) < 0.5, -1.0, 1.0)
    # |beta| in [0.5, 1]: a constant channel's y = beta is never at the ReLU edge, and neither is `twopoint`, whose y = beta +- 0.12 at most
    out = {"x": x, "dy": dy, "gamma": (sign() * (0.5 + rs.random_sample(C))).astype(np.float32),
           "beta": (sign() * (0.5 + 0.5 * rs.random_sample(C))).astype(np.float32),
           "rm0": rs.standard_normal(C).astype(np.float32), "rv0": (0.5 + rs.random_sample(C)).astype(np.float32),
           "base_g": rs.standard_normal(C).astype(np.float32), "base_b": rs.standard_normal(C).astype(np.float32)}
    combo = (np.arange(C) + idx * C) % (len(EVAL_VARS) * len(EVAL_MEANS))
    out["eval_rv"] = np.array(EVAL_VARS)[combo % len(EVAL_VARS)].astype(np.float32)
    out["eval_rm"] = np.array(EVAL_MEANS)[combo // len(EVAL_VARS)].astype(np.float32)
    out["eval_combo"] = combo
    if masked is not None:
        out["valid"] = valid
    for a in out.values():
        a.setflags(write=False)
    out["regimes"] = [regime_of(c) for c in range(C)]
    out["dy_regimes"] = [dy_regime_of(c, idx) for c in range(C)]
    _cache[key] = out
    return out


OUTPUTS = ("save_mean", "save_rstd", "running_mean", "running_var", "y", "dx", "dgamma", "dbeta")


def reference(t, relu=False, mask=None, acc=False):
    """(float64 results, bounds, forward dict) of a `make_case` dict, keyed by OUTPUTS.  mask: the ReLU mask the backward pass uses
    (default: the restatement's own y > 0); acc: dgamma / dbeta accumulate into base_g / base_b (beta_acc = 1)."""
    valid = t.get("valid")
    fwd = train_fwd(t["x"], t["gamma"], t["beta"], valid)
    keep = (fwd["y"] > 0 if mask is None else np.asarray(mask, dtype=bool)) if relu else np.ones(t["x"].shape, dtype=bool)
    bwd = train_bwd(fwd, t["gamma"], np.where(keep, t["dy"].astype(np.float64), 0.0), valid)
    base = (t["base_g"], t["base_b"]) if acc else None
    bnd = bounds(t["x"], t["gamma"], t["beta"], fwd, bwd, valid, t["rm0"], t["rv0"], base)
    rm, rv = running_update(t["rm0"], t["rv0"], fwd["mean"], fwd["var"], fwd["n"])
    ref = {"save_mean": fwd["mean"], "save_rstd": fwd["rstd"], "running_mean": rm, "running_var": rv, "y": fwd["y_relu" if relu else "y"],
           "dx": bwd["dx"], "dgamma": bwd["dgamma"] + (t["base_g"].astype(np.float64) if acc else 0.0),
           "dbeta": bwd["dbeta"] + (t["base_b"].astype(np.float64) if acc else 0.0)}
    return ref, bnd, fwd


def modelled(t, relu=False, acc=False):
    """kernel_model of a `make_case` dict, keyed by OUTPUTS"""
    return kernel_model(t["x"], t["gamma"], t["beta"], t["dy"], t.get("valid"), t["rm0"], t["rv0"], relu,
                        base=(t["base_g"], t["base_b"]) if acc else None)


REPLAY_MISMATCH = 1e-5       # share of elements a float64-emulated fma may round differently from a true one (2^-29 each, two fmas; 500x margin)
CONTROL_REL_L2 = 1e-5      # the suite's gate on dgamma / dbeta in the Gaussian regime, kept next to the bounds on the control channels


def control_channels(name):
    """channels of a case in the Gaussian regime of the existing suite: gauss x under gauss dy (not the shifted shards of the synchronised case)"""
    if name == SYNC_CASE:
        return []
    t = make_case(name)
    return [c for c, (a, b) in enumerate(zip(t["regimes"], t["dy_regimes"])) if (a, b) == ("gauss", "gauss")]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def ratio(err, bound):
    """max(err / bound) with 0 / 0 = 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q)) if q.size else 0.0


def channel_ratio(err, bound):
    """per channel max(err / bound) of (outer, C, inner) arrays"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return q.max(axis=(0, 2))
