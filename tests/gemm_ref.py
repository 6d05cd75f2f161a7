"""What every path of gemm.hip must compute, in numpy: operands whose product has no rounding in it, the expected values, the derived bound of
the generic family, NaN-framed buffers, and the table of cases (test_gemm_exact_host.py checks the claims made here on the CPU,
test_gemm_exact.py runs the table on the GPU).

C = op(A) op(B) + beta C0 with a logical A (M x K) and B (K x N); ta / tb only say how they are stored.

Family 1, integers.  Entries in [-7, 7]: every product and every partial sum is an integer below 2^24 (49 K + 128 < 2^24 up to K = 342 000), so
ANY kernel, k order, split-K and beta placement returns the float64 product exactly, at both precisions (|x| <= 7 is a bf16 value: lo = 0).

Family 2, two-level (precision 1).  a = p + q 2^-9 with p = +-{5, 6, 7}, |q| <= 7 (K <= 600) or p = +-3, |q| <= 3 (K <= 3 400).  |q| 2^-9 is
less than half a bf16 ulp of p (2^-6 in [4, 8), 2^-7 in [2, 4)) and p is no power of two (so p + q 2^-9 never leaves p's binade downwards, where
the ulp halves), hence split_bf16 gives hi = p, lo = q 2^-9 exactly, each of the three bf16x3 products is exact and every partial sum is a
multiple of 2^-9 below 2^15 (49 K 2^9 + 98 K + 2^16 = 15 177 136 at K = 600; 9 K 2^9 + 18 K + 2^16 = 15 791 936 at K = 3 400; 2^24 =
16 777 216).  The kernel must return  sum pa pb + 2^-9 sum (pa qb + qa pb)  bit for bit -- NOT the float64 product, which also has the
2^-18 sum qa qb that bf16x3 drops by design.  With gemm_bf16_single = 1 (hi * hi only): sum pa pb.

C0 holds multiples of 2^-8 with |C0| <= 64 and beta is one of 0, 1, 0.5, -2: beta C0 is an exact multiple of 2^-9 wherever it is applied.

Family 3, generic floats.  Gaussian entries (|g| floored at 2^-6 so that the scaled runs cannot underflow), rows of A and k rows of B scaled
by 2^U(-10, 10).  Against float64, per element:  |C - C64|_ij <= g (S_ij + |beta C0_ij|),  S_ij = sum_k |a_ik| |b_kj|,
  precision 0:  g = (K + splits + 2) 2^-24                                  (K float32 additions, the split-K reduce, beta C0 and its addition)
  precision 1:  g = 3 2^-16 (1 + 2^-7) + (K + splits + 2) 2^-24             (|x - hi - lo| <= 2^-16 |x| on each operand and the dropped lo lo
                                                                             term, |lo| <= 2^-8 |x|: three terms of 2^-16, second order 2^-7)
The bound is derived, not measured (the kernels sit between 0.01 and 0.43 of it: test_gemm_exact.py).  The same operands run again with row i of A times 2^e_i and column j
of B (and of C0: both) times 2^f_j, e, f in [-30, 30]: powers of two commute with the split, the products and the sums, nothing leaves
[2^-126, 2^127], so the result is the first one times 2^(e_i + f_j), bit for bit.
"""
import numpy as np

PATHS = ("f32", "f32_queue", "bf16x3", "planes128", "planes128_queue", "planes256", "planes256_af32", "planes256_queue", "tn")
NONE, ROWS, TR, TRQ = 0, 1, 2, 3                     # ctcn_diag_gemm_plan's split passes
BETAS = (0.0, 1.0, 0.5, -2.0)
F32 = np.float32


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as float32.  Finite inputs."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(F32)


def split_bf16(x):
    """gemm.hip's split_bf16: hi = bf16(x), lo = bf16(x - hi), the subtraction in float32."""
    x = np.ascontiguousarray(x, dtype=F32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


# ---- the generators -----------------------------------------------------------------------------------------------------------------
def integers(rs, shape):
    return rs.randint(-7, 8, shape).astype(F32)


def two_level_ranges(K):
    """(values of |p|, largest |q|) of the two-level family at contraction length K."""
    if K <= 600:
        return (5, 6, 7), 7
    assert K <= 3400, "the two-level family is exact up to K = 3 400"
    return (3,), 3


def two_level(rs, shape, K):
    """x = p + q 2^-9 as float32, with p and q."""
    ps, qmax = two_level_ranges(K)
    p = rs.choice(ps, shape).astype(F32) * rs.choice((-1.0, 1.0), shape).astype(F32)
    q = rs.randint(-qmax, qmax + 1, shape).astype(F32)
    return p + q * F32(2.0 ** -9), p, q


def c0_values(rs, shape):
    return (rs.randint(-64 * 256, 64 * 256 + 1, shape) / 256.0).astype(F32)


def gaussian(rs, M, N, K):
    """A (M x K), B (K x N), C0 (M x N) of the generic family."""
    def g(shape):
        v = rs.standard_normal(shape)
        return (np.sign(v) + (v == 0)) * np.maximum(np.abs(v), 2.0 ** -6)
    A = (g((M, K)) * np.exp2(rs.uniform(-10, 10, (M, 1)))).astype(F32)
    B = (g((K, N)) * np.exp2(rs.uniform(-10, 10, (K, 1)))).astype(F32)
    C0 = (g((M, N)) * (float(np.abs(A).max(initial=1.0)) * float(np.abs(B).max(initial=1.0)))).astype(F32)
    return A, B, C0


def pow2_scales(rs, M, N):
    """2^e_i (M x 1) and 2^f_j (1 x N), e, f integers in [-30, 30]."""
    return np.exp2(rs.randint(-30, 31, (M, 1))).astype(F32), np.exp2(rs.randint(-30, 31, (1, N))).astype(F32)


# ---- expected values ----------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64)      # (float64 BLAS: the integer sums stay below 2^53)


def expected_integers(A, B):
    return _mm(A, B)


def expected_two_level(pa, qa, pb, qb, single=False):
    if single:
        return _mm(pa, pb)
    return _mm(pa, pb + qb * 2.0 ** -9) + _mm(qa, pb) * 2.0 ** -9


def with_beta(prod, C0, beta):
    """float64 product + beta C0 -> float32; `exact` says whether the conversion lost nothing."""
    v = prod + 0.0                         # (an accumulator starts at +0: a sum of -0 terms is +0 in the kernels)
    if beta != 0.0:
        v = v + float(beta) * C0.astype(np.float64)
    out = v.astype(F32)
    return out, bool(np.array_equal(out.astype(np.float64), v))


def bound_g(K, splits, prec):
    g = (K + splits + 2) * 2.0 ** -24
    return g + 3 * 2.0 ** -16 * (1 + 2.0 ** -7) if prec == 1 else g


def shift_rows(B, shift):
    """ctcn_gemm_shift_b's operand: row k takes row k - shift of B where that exists, zero otherwise."""
    out = np.zeros_like(B)
    K = B.shape[0]
    if shift >= 0:
        out[shift:] = B[:K - shift]
    else:
        out[:K + shift] = B[-shift:]
    return out


# ---- float32 emulation of bf16x3 (and of its mutants) -------------------------------------------------------------------------------
def emulate_bf16x3(A, B, C0=None, beta=0.0, order=None, chunks=1, mutant=None, single=False):
    """float32 accumulation, per k in `order`: lo*hi, hi*lo, hi*hi; the k list cut into `chunks` split-K partials that are summed in order, then
    beta C0.  mutant: "drop_lo_hi" | "drop_hi_lo" | "add_lo_lo" | "shift_lo" (A's lo plane one k late) | "drop_last_k" | "beta_twice"."""
    M, K = A.shape
    N = B.shape[1]
    ah, al = split_bf16(A)
    bh, bl = split_bf16(B)
    if mutant == "shift_lo":
        al = np.concatenate([np.zeros((M, 1), F32), al[:, :-1]], axis=1)
    ks = list(range(K) if order is None else order)
    if mutant == "drop_last_k":
        ks = [k for k in ks if k != K - 1]
    parts = []
    for chunk in np.array_split(np.asarray(ks, dtype=np.int64), chunks):
        acc = np.zeros((M, N), F32)
        for k in chunk:
            if not single:
                if mutant != "drop_lo_hi":
                    acc = acc + np.outer(al[:, k], bh[k])
                if mutant != "drop_hi_lo":
                    acc = acc + np.outer(ah[:, k], bl[k])
            acc = acc + np.outer(ah[:, k], bh[k])
            if mutant == "add_lo_lo":
                acc = acc + np.outer(al[:, k], bl[k])
        parts.append(acc)
    out = np.zeros((M, N), F32)
    for p in parts:
        out = out + p
    if beta != 0.0:
        out = out + F32(beta) * C0
        if mutant == "beta_twice":
            out = out + F32(beta) * C0
    assert out.dtype == F32
    return out


MUTANTS = ("drop_lo_hi", "drop_hi_lo", "add_lo_lo", "shift_lo", "drop_last_k", "beta_twice")
# the integer family has lo = 0: the mutants that only move lo terms cannot show on it
MUTANTS_INTEGERS = ("drop_last_k", "beta_twice")


# ---- NaN frames ---------------------------------------------------------------------------------------------------------------------
GUARD = 3


def frame(mat, ld, fill=np.nan, col0=0):
    """`mat` (rows x cols) as a window of leading dimension ld inside a flat float32 buffer of `fill`: GUARD rows of ld before and after, the row
    padding filled too.  Returns (flat buffer, offset of the window's first element)."""
    rows, cols = mat.shape
    assert ld >= cols + col0
    buf = np.full((rows + 2 * GUARD) * ld, fill, F32)
    off = GUARD * ld + col0
    if rows and cols:
        np.lib.stride_tricks.as_strided(buf[off:], (rows, cols), (4 * ld, 4))[...] = mat
    return buf, off


def window(buf, off, rows, cols, ld):
    return np.lib.stride_tricks.as_strided(buf[off:], (rows, cols), (4 * ld, 4))


def stored(mat, trans):
    """The logical operand as it lies in memory: A is stored K x M when ta, B is stored N x K when tb."""
    return np.ascontiguousarray(mat.T) if trans else mat


def leading_dims(case, pad):
    """(lda, ldb, ldc) of a case at row padding `pad`; a case that fixes lda / ldb keeps them."""
    ta, tb, M, N, K = case["shape"]
    lda = case.get("lda") or (M if ta else K) + pad
    ldb = case.get("ldb") or (K if tb else N) + pad
    return lda, ldb, N + pad


def mod16(ld, col0=0):
    """Byte offset modulo 16 of a frame's window in a 16-byte aligned buffer."""
    return (GUARD * ld + col0) * 4 % 16


# ---- the table ----------------------------------------------------------------------------------------------------------------------
# One row per product: shape = (ta, tb, M, N, K); prec; what moves from the defaults -- xcd (side-stream mask), opts (ctcn_set_option), ws
# ("main": the stream's workspace, None: no workspace, an int: a private workspace of that many bytes), lda / ldb where the row fixes them,
# entry ("gemm": ctcn_gemm / ctcn_diag_gemm_on_xcds, "dx": ctcn_gemm_dx) -- and the plan it must take on a device of 256 CUs in 8 XCDs with
# rows padded by 4 floats: (path, tile / 64, wnt, splits, split pass of A, of B).  plan1: (path, splits) with rows padded by ONE float (every
# row but each fourth off 16 bytes), where that differs: such rows leave the float32-A tile, the TN tile and the 256 x 320 tile, which is the
# point of running them.  Shapes are the issue's; none had to move.  Rows marked + come from test_host_logic.test_gemm_plan_table.
def _case(path, prec, shape, plan, plan1=None, **kw):
    d = dict(path=path, prec=prec, shape=shape, plan=(path,) + plan, plan1=plan1, xcd=0, opts={}, ws="main", entry="gemm", single=False)
    d.update(kw)
    tag = "".join("%s%s" % (k, v) for k, v in sorted(d["opts"].items()))
    d["id"] = "%s-p%d-%d%d-%dx%dx%d%s%s%s%s" % (path if d["entry"] == "gemm" else "dx_wide", prec, *shape, "-xcd%x" % d["xcd"] if d["xcd"] else "",
                                               "-" + tag if tag else "", "" if d["ws"] == "main" else "-ws%s" % d["ws"],
                                               "-ld%d_%d" % (d["lda"], d["ldb"]) if d.get("lda") else "")
    return d


def _table():
    t = []
    D = ((2, 2), 0, 1, NONE, NONE)                      # the direct kernels: 128 x 128 tile, one K sweep
    for ta in (0, 1):
        for tb in (0, 1):
            pa, pb = (TR if ta else ROWS), (ROWS if tb else TR)
            for M, N, K in ((1, 1, 1), (33, 17, 5), (129, 130, 3), (128, 128, 16), (200, 62, 40), (33, 17, 0), (33, 17, 1)):
                t.append(_case("f32", 0, (ta, tb, M, N, K), D))
            t.append(_case("bf16x3", 1, (ta, tb, 33, 17, 5), D))
            for K in (0, 1, 3):
                t.append(_case("bf16x3", 1, (ta, tb, 33, 17, K), D))
            t.append(_case("planes128", 1, (ta, tb, 300, 257, 130), ((2, 2), 0, 1, pa, pb)))
    t += [
        _case("f32", 0, (0, 1, 33, 17, 512), ((2, 2), 0, 2, NONE, NONE)),                       # split-K
        _case("f32", 0, (1, 0, 33, 17, 515), ((2, 2), 0, 2, NONE, NONE)),                       # ... a tail in the last chunk (288 + 227)
        _case("f32_queue", 0, (0, 0, 200, 62, 40), D, xcd=0x01),                                # +
        _case("bf16x3", 1, (0, 1, 200, 62, 40), D),
        _case("bf16x3", 1, (1, 0, 200, 62, 40), D),
        _case("bf16x3", 1, (0, 1, 2048, 256, 63), D),                                           # +
        _case("bf16x3", 1, (0, 1, 300, 257, 130), D, ws=None),                                  # no workspace
        _case("bf16x3", 1, (1, 0, 64, 64, 1024), ((2, 2), 0, 4, NONE, NONE), ws=65536),         # planes do not fit, four partials do
        _case("planes128", 1, (0, 1, 2048, 256, 64), ((2, 2), 0, 1, ROWS, ROWS)),               # +
        _case("planes128", 1, (0, 1, 2048, 256, 65), ((2, 2), 0, 1, ROWS, ROWS)),
        _case("planes128", 1, (1, 0, 128, 64, 1023), ((2, 2), 0, 2, TR, TR)),                   # + split-K
        _case("planes128", 1, (0, 1, 8192, 1024, 200), ((2, 4), 0, 1, ROWS, ROWS), opts=dict(gemm_big_tiles=1)),   # +
        _case("planes128_queue", 1, (1, 1, 300, 257, 130), ((2, 2), 0, 1, TRQ, ROWS), xcd=0xF0),                  # +
        _case("planes128_queue", 1, (0, 0, 300, 257, 130), ((2, 2), 0, 1, ROWS, TRQ), xcd=0xF0),                  # +
        _case("planes256", 1, (0, 1, 1024, 16384, 128), ((4, 4), 2, 1, ROWS, ROWS)),            # +
        _case("planes256", 1, (1, 1, 49152, 96, 128), ((4, 2), 1, 1, TR, ROWS)),                # A through the transposing split
        _case("planes256", 1, (0, 1, 16390, 1030, 200), ((4, 2), 1, 1, ROWS, ROWS)),            # + ragged M and N
        _case("planes256_af32", 1, (0, 0, 49152, 96, 128), ((4, 2), 1, 1, NONE, TR), plan1=("planes256", 1)),     # +
        _case("planes256_af32", 1, (0, 1, 49152, 256, 128), ((4, 4), 2, 1, NONE, ROWS), plan1=("planes256", 1)),  # +
        _case("planes256_af32", 1, (0, 0, 49153, 96, 100), ((4, 2), 1, 1, NONE, TR), plan1=("planes256", 1)),     # K % 32 != 0, ragged M
        _case("planes256_queue", 1, (0, 1, 6144, 128, 64), ((4, 2), 1, 1, ROWS, ROWS), xcd=0x01),                 # +
        _case("tn", 1, (1, 0, 128, 64, 1024), ((4, 2), 1, 2, NONE, NONE), plan1=("planes128", 2)),                # +
        _case("tn", 1, (1, 0, 128, 32, 1024), ((4, 2), 1, 2, NONE, NONE), plan1=("planes128", 2)),                # +
        _case("tn", 1, (1, 0, 128, 64, 1027), ((4, 2), 1, 2, NONE, NONE), plan1=("planes128", 2)),
        _case("tn", 1, (1, 0, 388, 132, 1100), ((4, 4), 2, 2, NONE, NONE), lda=396, ldb=140),
        _case("tn", 1, (1, 0, 388, 132, 1100), ((4, 4), 2, 3, NONE, NONE), lda=396, ldb=140, opts=dict(tn_splits_force=3)),   # +
        _case("tn", 1, (1, 0, 388, 132, 1100), ((4, 4), 2, 2, NONE, NONE), lda=396, ldb=140, xcd=0x01),                       # +
        # ctcn_gemm_dx's 256 x 320 tile: no plan_gemm path of its own (ctcn_diag_dx_plan says `wide`); rows off 16 bytes go to ctcn_gemm(0, 0)
        _case("planes128", 1, (0, 0, 256, 320, 64), ((2, 2), 0, 1, ROWS, TR), entry="dx", opts=dict(gemm_dx_wide=2)),
        _case("planes128", 1, (0, 0, 513, 640, 100), ((2, 2), 0, 1, ROWS, TR), entry="dx", opts=dict(gemm_dx_wide=2)),
        # gemm_bf16_single = 1 on the 256-row tiles: hi * hi alone
        _case("planes256", 1, (0, 1, 1024, 16384, 128), ((4, 4), 2, 1, ROWS, ROWS), opts=dict(gemm_bf16_single=1), single=True),
        _case("planes256", 1, (1, 1, 49152, 96, 128), ((4, 2), 1, 1, TR, ROWS), opts=dict(gemm_bf16_single=1), single=True),
        _case("planes256_af32", 1, (0, 0, 49152, 96, 128), ((4, 2), 1, 1, NONE, TR), plan1=("planes256", 1), opts=dict(gemm_bf16_single=1), single=True),
        _case("planes256_af32", 1, (0, 1, 49152, 256, 128), ((4, 4), 2, 1, NONE, ROWS), plan1=("planes256", 1), opts=dict(gemm_bf16_single=1),
              single=True),
    ]
    ids = [c["id"] for c in t]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return t


CASES = _table()


def plan_args(case, pad):
    """Arguments of test_host_logic._gemm_plan for a case at row padding `pad` (operands framed by frame(): their offsets modulo 16 bytes)."""
    ta, tb, M, N, K = case["shape"]
    lda, ldb, _ = leading_dims(case, pad)
    ws = case["ws"]
    return (ta, tb, M, N, K), dict(prec=case["prec"], lda=lda, ldb=ldb, amod=mod16(lda), bmod=mod16(ldb), xcd=case["xcd"],
                                   **({} if ws == "main" else {"ws": ws}))


def plan_tuple(d):
    return (d["path"], (d["ti"], d["tj"]), d["wnt"], d["splits"], d["split_a"], d["split_b"])


def expected_plan(case, pad):
    """The whole plan at pad 4; (path, splits) at pad 1."""
    if pad == 4:
        return case["plan"]
    return case["plan1"] or (case["plan"][0], case["plan"][3])


def combos(case):
    """(family, pad, beta) runs of a case.  The exact families: every beta at padding 4 (the path the row names), and at padding 1 every beta on
    the small products, two on the large ones (M N > 2^17: beta = 0 -- the window starts as NaN -- and one more).  The generic family: one
    run per padding."""
    ta, tb, M, N, K = case["shape"]
    fams = ["int"] + (["two"] if case["prec"] == 1 else []) + ([] if case["single"] else ["gauss"])
    out = []
    for f in fams:
        if f == "gauss":
            out += [(f, 4, 1.0), (f, 1, 0.0)]
        else:
            out += [(f, 4, b) for b in BETAS] + [(f, 1, b) for b in (BETAS if M * N <= 1 << 17 else (0.0, 0.5 if f == "int" else -2.0))]
    return out


class set_options:
    """with set_options(dict(name=value)): ctcn_set_option for the block, the former values put back after it."""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from ctc_pytorch_amd import ops
        self.old = {n: ops.get_option(n) for n in self.opts}
        for n, v in self.opts.items():
            ops.set_option(n, v)

    def __exit__(self, *a):
        from ctc_pytorch_amd import ops
        for n, v in self.old.items():
            ops.set_option(n, v)


# ctcn_gemm_shift_b and GemmPlanes::same_a through ctcn_diag_gemm_shift_b_pair: (M, N, K, shifts); lda = 2 M, ldb = 2 N (the two directions of a
# bidirectional layer side by side).  N = 16: split_transpose_tile's scalar branch, 64: one 16-byte tile, 80: one of each.
def _shifts(K):
    return [s * sg for s in (1, 8, 16, 64, 65, K - 1) for sg in (1, -1)]


SHIFT_CASES = [(64, N, K, _shifts(K)) for N in (16, 64, 80) for K in (192, 200)]
SHIFT_TN_CASE = (128, 32, 1100, (16, -16))             # the narrowed window (K - 16 = 1 084) goes to the TN tile: the pointer-offset branch
