"""float64 restatement of the Adam update, a float32 replay of the kernels' expression, and derived bounds  --  TEST INFRASTRUCTURE ONLY
(used by test_adam_regimes*.py).

REFERENCE (`step`): torch.optim.Adam's formula in float64, with beta1, beta2, lr, eps the float32 values the ABI receives --
    g' = clip g + wd p;   m' = b1 m + (1 - b1) g';   v' = b2 v + (1 - b2) g'^2;   p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
(clip = 1 for ctcn_adam_step; for ctcn_adam_step_ex the float32 coefficient of the control block).  tests/test_adam_regimes_host.py holds it to
torch.optim.Adam in float64.

KERNEL EXPRESSION (`replay`; adam_kernel / adam_ex_kernel in csrc/elementwise.hip), every operation in float32:
    gv = fma(wd, p, fl(g clip));   mv = fl(fl(b1 m) + fl(fl(1 - b1) gv));   vv = fl(fl(b2 v) + fl(fl(fl(1 - b2) gv) gv))
    p' = fl(p - fl(step_size fl(mv / fl(fl(sqrtf(vv) / sqrt_bc2) + eps)))),   step_size = fl32(lr / (1 - b1^t)), sqrt_bc2 = fl32(sqrt(1 - b2^t))
adam_kernel leaves the contraction of a * b + c to the compiler; a fused operation rounds once where the replay rounds twice, so the bounds
below, which count every rounding of the replay, hold for either.

BOUNDS (`bounds`), u = 2^-24, by running error analysis of that expression; F = 2^-126 is added to every float32 result (a result below the
normal range may be flushed or rounded to the subnormal spacing: either is allowed):
    1 - b1, 1 - b2   exact in float32 (Sterbenz) and equal to the float64 value
    g'    e = u |g clip| [clip != 1] + u |g'|
    m'    u (|b1 m| + |(1 - b1) g'|) (the two products) + (1 - b1) e(g') + u |m'| (the sum): 3 roundings; the terms may cancel, so the bound is
          relative to the terms, not to m'
    v'    u b2 v + 2 u (1 - b2) g'^2 + 2 (1 - b2) |g'| e(g') + (1 - b2) e(g')^2 + u v': 4 roundings, nothing cancels
    s = sqrtf(v')   the interval [sqrt(max(v' - e, 0)), sqrt(v' + e)] (v' may be 0 within its floor) + u s
    q = s / sqrt_bc2   sqrt_bc2 carries one float32 rounding: e(q) = (e(s) + u s) / sqrt_bc2 + u q
    D = q + eps       e(D) = e(q) + u D;   D >= eps > e(D)
    r = m' / D        e(r) = e(m') / (D - e(D)) + |m'| e(D) / (D (D - e(D))) + u |r|
    dp = step_size r  step_size carries one float32 rounding: e(dp) = (lr / bc1) (e(r) + u |r|) (1 + u) + u |dp|
    p'    e(dp) + u |p'|, i.e. relative to |dp|, plus half an ulp of p', plus what m' and v' carry
The square root and the division are taken as correctly rounded (hipcc's default for float32).
"""
import numpy as np

U = 2.0 ** -24
F = 2.0 ** -126
B1, B2, EPS = (float(np.float32(v)) for v in (0.9, 0.999, 1e-8))
LRS = (1e-3, 1e-6)
WDS = (0.0, 5e-4)
# the issue's five step counts, and 10 000: the largest of them at which 1 - beta2^t still differs from 1 (by 4.5e-5; at 100 000 by 4e-44)
STEPS = (1, 2, 10, 1000, 10000, 100000)
N = 4099
f32v = lambda v: float(np.float32(v))


def corrections(t, lr, b1=B1, b2=B2):
    """(lr / (1 - b1^t), sqrt(1 - b2^t)) in float64"""
    return lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)


def step(p, g, m, v, t, lr, wd, clip=1.0, b1=B1, b2=B2, eps=EPS):
    """(p', m', v') in float64"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    ss, sbc = corrections(t, lr, b1, b2)
    g1 = g * clip + wd * p
    m1 = b1 * m + (1.0 - b1) * g1
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    return p - ss * (m1 / (np.sqrt(v1) / sbc + eps)), m1, v1


def _r(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def replay(p, g, m, v, t, lr, wd, clip=1.0, b1=B1, b2=B2, eps=EPS, step_size=None, sqrt_bc2=None):
    """the kernels' expression, one float32 rounding per operation (float64 arrays holding float32 values)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    ss, sbc = corrections(t, lr, b1, b2)
    ss = float(_r(ss)) if step_size is None else step_size
    sbc = float(_r(sbc)) if sqrt_bc2 is None else sqrt_bc2
    gv = _r(wd * p + _r(g * clip))
    mv = _r(_r(b1 * m) + _r(_r(1.0 - b1) * gv))
    vv = _r(_r(b2 * v) + _r(_r(_r(1.0 - b2) * gv) * gv))
    with np.errstate(invalid="ignore", divide="ignore"):
        p1 = _r(p - _r(ss * _r(mv / _r(_r(_r(np.sqrt(vv)) / sbc) + eps))))
    return p1, mv, vv


def bounds(p, g, m, v, t, lr, wd, clip=1.0, b1=B1, b2=B2, eps=EPS):
    """{p, m, v}: bounds on |device - step(...)| (module docstring)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    p1, m1, v1 = step(p, g, m, v, t, lr, wd, clip, b1, b2, eps)
    ss, sbc = corrections(t, lr, b1, b2)
    g1 = g * clip + wd * p
    e_g = (U * np.abs(g * clip) if clip != 1.0 else 0.0) + U * np.abs(g1) + F
    e_m = U * (np.abs(b1 * m) + np.abs((1.0 - b1) * g1)) + (1.0 - b1) * e_g * (1 + U) + U * np.abs(m1) + 3 * F
    e_v = U * b2 * v + 2 * U * (1.0 - b2) * g1 * g1 + (2 * (1.0 - b2) * np.abs(g1) * e_g + (1.0 - b2) * e_g ** 2) * (1 + 2 * U) + U * v1 + 4 * F
    s = np.sqrt(v1)
    e_s = np.maximum(np.sqrt(v1 + e_v) - s, s - np.sqrt(np.maximum(v1 - e_v, 0.0))) + U * (s + np.sqrt(e_v)) + F
    q = s / sbc
    e_q = (e_s + U * (s + e_s)) / sbc * (1 + U) + U * q + F
    d = q + eps
    e_d = e_q + U * (d + e_q) + F
    assert np.all(e_d < 0.5 * d)
    r = m1 / d
    e_r = e_m / (d - e_d) + np.abs(m1) * e_d / (d * (d - e_d)) + U * (np.abs(r) + e_m / (d - e_d)) + F
    dp = ss * r
    e_dp = ss * (1 + U) * (e_r + U * (np.abs(r) + e_r)) + U * np.abs(dp) + F
    e_dp = e_dp + U * e_dp
    return {"p": e_dp + U * (np.abs(p1) + e_dp) + F, "m": e_m, "v": e_v}


# ---------------------------------------------------------------------------------------------------------------------------------
# the sweep: single steps from a designed state
# ---------------------------------------------------------------------------------------------------------------------------------
P_VALUES = (0.0, 1e-3, -1e-3, 1.0, -1.0, 1e4, -1e4)


def _grid(rs, n, kmin, kmax, signed, zero_share):
    """{0, (+-) a 2^k}: a on a 12-bit significand grid in [1, 2), k uniform in [kmin, kmax]"""
    a = (1.0 + rs.randint(0, 2 ** 11, size=n) / 2.0 ** 11) * 2.0 ** rs.randint(kmin, kmax + 1, size=n)
    if signed:
        a = a * np.where(rs.random_sample(n) < 0.5, -1.0, 1.0)
    return np.where(rs.random_sample(n) < zero_share, 0.0, a)


def sweep_state(seed=0, n=N):
    """{p, g, m, v}: float32 arrays of n elements (one odd tail), the axes crossed at random --
    g in {0, +-2^k}, k = -60 .. 40;  v in {0, 2^k}, k = -120 .. 80;  m in {0, +- the scale of g or of sqrt(v), times 2^-3 .. 2^3};  p in P_VALUES"""
    rs = np.random.RandomState(31337 + seed)
    g = _grid(rs, n, -60, 40, True, 0.08)
    v = _grid(rs, n, -120, 80, False, 0.1)
    scale = np.where(rs.random_sample(n) < 0.5, np.abs(g), np.sqrt(v))
    scale = np.where(scale == 0, np.maximum(np.abs(g), np.sqrt(v)), scale)
    scale = 2.0 ** np.floor(np.log2(np.where(scale == 0, 1.0, scale))) * (scale != 0)
    m = scale * _grid(rs, n, -3, 3, True, 0.1)
    p = np.array(P_VALUES)[rs.randint(0, len(P_VALUES), size=n)]
    out = {"p": p, "g": g, "m": m, "v": v}
    for k in out:
        a32 = out[k].astype(np.float32)
        assert k == "p" or np.array_equal(a32.astype(np.float64), out[k])          # the grids are exact in float32
        out[k] = a32
        out[k].setflags(write=False)
    return out


def sweep_calls():
    """[(step, lr, wd)]: the per-call axes, crossed"""
    return [(t, f32v(lr), f32v(wd)) for t in STEPS for lr in LRS for wd in WDS]


def multi_step_data(steps=200, n=10007, seed=5):
    """(p0 float32, [g_t float32]): gradients log-uniform in magnitude over 1e-10 .. 1e-2, random signs, 5 % exact zeros"""
    rs = np.random.RandomState(seed)
    p0 = rs.standard_normal(n).astype(np.float32)
    gs = []
    for _ in range(steps):
        mag = 10.0 ** rs.uniform(-10.0, -2.0, size=n) * np.where(rs.random_sample(n) < 0.5, -1.0, 1.0)
        gs.append(np.where(rs.random_sample(n) < 0.05, 0.0, mag).astype(np.float32))
    return p0, gs


def multi_step_reference(p0, gs, lr, wd):
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    for t, g in enumerate(gs, 1):
        p, m, v = step(p, g, m, v, t, lr, wd)
    return p


def ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q))
