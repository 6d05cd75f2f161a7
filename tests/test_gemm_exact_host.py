"""CPU checks of tests/gemm_ref.py, the reference test_gemm_exact.py holds gemm.hip to on the GPU.  Nothing here runs a kernel:

  1. the generators keep their promises for every row of the table (split_bf16 of a two-level operand is exactly (p, q 2^-9); the sum of
     the terms' magnitudes plus |beta C0| stays below 2^24 units; the scaled generic family stays inside [2^-100, 2^100]);
  2. a float32 emulation of bf16x3 (lo*hi, hi*lo, hi*hi per k, k shuffled, 2 to 4 split-K partials) reproduces the expected values of the two
     exact families bit for bit -- the expectation does not depend on an order;
  3. every mutant of the emulation (a product dropped, lo*lo added, A's lo plane one k late, the last k dropped, beta applied twice) changes at
     least one output: the operands discriminate;
  4. the emulation stays within the derived bound g on the generic family, and its power-of-two scaled run is the first one scaled;
  5. ctcn_diag_gemm_plan on 256 CUs in 8 XCDs sends every row of the table to the path, tile, wnt, split-K count and split passes the table
     names, at both row paddings, and the shifted / reused products to the plane path without A's split pass.

The large products are checked on a sample of their rows and columns (first, last and random ones) over the whole of K.
"""
import ctypes
import zlib

import numpy as np
import pytest

import gemm_ref as R
from test_host_logic import _gemm_plan

ROWS_SAMPLE, COLS_SAMPLE = 24, 20


def seed_of(case):
    return zlib.crc32(case["id"].encode()) & 0x7FFFFFFF


def sample(n, m, rs):
    if n <= m:
        return np.arange(n)
    return np.unique(np.concatenate([[0, n - 1], rs.choice(n, m - 2, replace=False)]))


def sampled(case):
    """(M', N', K, rs) of a case cut down to a sample of its rows and columns: the generators are elementwise, so a smaller draw is as good."""
    ta, tb, M, N, K = case["shape"]
    return min(M, ROWS_SAMPLE), min(N, COLS_SAMPLE), K, np.random.RandomState(seed_of(case))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_generators_keep_their_promises(case):
    ta, tb, M, N, K = case["shape"]
    rs = np.random.RandomState(seed_of(case))
    rows, cols = sample(M, 512, rs), sample(N, 512, rs)
    m, n = len(rows), len(cols)
    unit = 2.0 ** 24
    # integers: |x| <= 7, exact in bf16; sum |a| |b| + |beta C0| < 2^24
    A, B, C0 = R.integers(rs, (m, K)), R.integers(rs, (K, n)), R.c0_values(rs, (m, n))
    for X in (A, B):
        hi, lo = R.split_bf16(X)
        assert np.array_equal(hi, X) and not lo.any() and np.abs(X).max(initial=0) <= 7
    assert np.array_equal(C0 * 256, np.round(C0 * 256)) and np.abs(C0).max() <= 64
    assert 49 * K + 2 * 64 < unit
    assert (np.abs(A).astype(np.float64) @ np.abs(B) + 2 * np.abs(C0)).max() < unit
    if case["prec"] == 1:
        (A, pa, qa), (B, pb, qb) = R.two_level(rs, (m, K), K), R.two_level(rs, (K, n), K)
        ps, qmax = R.two_level_ranges(K)
        for X, p, q in ((A, pa, qa), (B, pb, qb)):
            hi, lo = R.split_bf16(X)
            assert np.array_equal(hi, p) and np.array_equal(lo, q * np.float32(2.0 ** -9))
            assert np.array_equal(X.astype(np.float64), p.astype(np.float64) + q * 2.0 ** -9)       # p + q 2^-9 is a float32
            assert set(np.abs(p).ravel().tolist()) <= set(float(v) for v in ps) and np.abs(q).max(initial=0) <= qmax
        # every term and every partial sum is a multiple of 2^-9; the magnitudes, in units of 2^-9, stay below 2^24
        pm = max(ps)
        assert (pm * pm * K * 512 + 2 * pm * qmax * K + 2 * 64 * 512) < unit
        S = np.abs(pa).astype(np.float64) @ (np.abs(pb) + np.abs(qb) * 2.0 ** -9) + (np.abs(qa).astype(np.float64) @ np.abs(pb)) * 2.0 ** -9
        assert ((S + 2 * np.abs(C0)) * 512).max() < unit
        for beta in R.BETAS:
            want, exact = R.with_beta(R.expected_two_level(pa, qa, pb, qb), C0, beta)
            assert exact and np.array_equal(want * 512, np.round(want * 512))
            if K:          # it is not the float64 product: that one also has 2^-18 sum qa qb
                assert not np.array_equal(R.expected_two_level(pa, qa, pb, qb), R._mm(A, B))
    if not case["single"]:
        A, B, C0 = R.gaussian(rs, m, n, K)
        sa, sb = R.pow2_scales(rs, m, n)
        for X in (A * sa, B * sb, C0 * sa * sb):
            assert np.isfinite(X).all()
            if X.size:
                assert 2.0 ** -100 <= np.abs(X).min() and np.abs(X).max() <= 2.0 ** 100
        if K:
            lo, hi = np.abs(A * sa).astype(np.float64), np.abs(B * sb).astype(np.float64)
            assert lo.min() * hi.min() >= 2.0 ** -100 and lo.max() * hi.max() * K <= 2.0 ** 100


def families(case, m, n, K, rs):
    """name -> (A, B, C0, float64 product expected of bf16x3 (of the hi planes alone for a `single` case))."""
    out = {}
    A, B = R.integers(rs, (m, K)), R.integers(rs, (K, n))
    out["int"] = (A, B, R.c0_values(rs, (m, n)), R.expected_integers(A, B))
    if case["prec"] == 1:
        (A, pa, qa), (B, pb, qb) = R.two_level(rs, (m, K), K), R.two_level(rs, (K, n), K)
        out["two"] = (A, B, R.c0_values(rs, (m, n)), R.expected_two_level(pa, qa, pb, qb, single=case["single"]))
    return out


@pytest.mark.parametrize("case", [c for c in R.CASES if c["prec"] == 1], ids=lambda c: c["id"])
def test_emulation_reproduces_the_expected_values_in_any_order(case):
    m, n, K, rs = sampled(case)
    for name, (A, B, C0, prod) in families(case, m, n, K, rs).items():
        for i, beta in enumerate(R.BETAS):
            want, exact = R.with_beta(prod, C0, beta)
            assert exact
            got = R.emulate_bf16x3(A, B, C0, beta, order=rs.permutation(K), chunks=2 + (i + K) % 3, single=case["single"])
            assert np.array_equal(got, want), (name, beta)
        assert np.array_equal(R.emulate_bf16x3(A, B, single=case["single"]), R.with_beta(prod, C0, 0.0)[0])


@pytest.mark.parametrize("case", [c for c in R.CASES if c["prec"] == 1 and not c["single"]], ids=lambda c: c["id"])
def test_every_mutant_changes_an_output(case):
    m, n, K, rs = sampled(case)
    for name, (A, B, C0, prod) in families(case, m, n, K, rs).items():
        want = R.with_beta(prod, C0, 0.5)[0]
        for mutant in (R.MUTANTS if name == "two" else R.MUTANTS_INTEGERS):
            if K == 0 and mutant != "beta_twice":
                continue                                  # nothing to drop or move in an empty sum
            got = R.emulate_bf16x3(A, B, C0, 0.5, mutant=mutant)
            assert not np.array_equal(got, want), (name, mutant)


@pytest.mark.parametrize("case", [c for c in R.CASES if c["prec"] == 1 and not c["single"]], ids=lambda c: c["id"])
def test_emulation_within_the_bound_and_scale_invariant(case):
    m, n, K, rs = sampled(case)
    A, B, C0 = R.gaussian(rs, m, n, K)
    sa, sb = R.pow2_scales(rs, m, n)
    S = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    for beta, chunks in ((0.0, 1), (1.0, 3)):
        got = R.emulate_bf16x3(A, B, C0, beta, chunks=chunks)
        err = np.abs(got.astype(np.float64) - (R._mm(A, B) + beta * C0.astype(np.float64)))
        bound = R.bound_g(K, chunks, 1) * (S + abs(beta) * np.abs(C0))
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        scaled = R.emulate_bf16x3(A * sa, B * sb, C0 * sa * sb, beta, chunks=chunks)
        assert np.array_equal(scaled, got * sa * sb)


def dx_plan(M, N, K, lda, amod):
    from ctc_pytorch_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.lib().ctcn_diag_dx_plan(M, N, K, lda, 1, amod, 1, 1 << 30, 256, ctypes.cast(out, ctypes.c_void_p)) == 0
    return dict(eligible=out[0], wide=out[1])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_table_rows_take_the_paths_they_name(case):
    with R.set_options(case["opts"]):
        for pad in (4, 1):
            a, k = R.plan_args(case, pad)
            got = _gemm_plan(*a, **k)
            want = R.expected_plan(case, pad)
            assert (R.plan_tuple(got) if pad == 4 else (got["path"], got["splits"])) == want, (pad, got)
            if case["entry"] == "dx":
                ta, tb, M, N, K = case["shape"]
                assert dx_plan(M, N, K, k["lda"], k["amod"]) == (dict(eligible=1, wide=1) if pad == 4 else dict(eligible=0, wide=0))
    assert case["plan"][0] == case["path"] and case["path"] in R.PATHS


def test_shifted_and_reused_products_take_the_plane_path():
    """ctcn_gemm_shift_b's choice, restated: the whole window on the plane path (B shifted while it is split; with same_a, no split pass of A)
    unless the narrowed window would go to the TN tile; at precision 0 there are no planes and the window is narrowed."""
    for M, N, K, shifts in R.SHIFT_CASES:
        for s in shifts:
            kw = dict(lda=2 * M, ldb=2 * N, shift=s)
            for xcd, tr in ((0, R.TR), (0xF0, R.TRQ)):
                assert R.plan_tuple(_gemm_plan(1, 0, M, N, K, xcd=xcd, **kw)) == ("planes128" + ("_queue" if xcd else ""), (2, 2), 0, 1, tr, tr)
                assert R.plan_tuple(_gemm_plan(1, 0, M, N, K, xcd=xcd, same_a=1, **kw))[4:] == (R.NONE, tr)
            assert _gemm_plan(1, 0, M, N, K - abs(s), lda=2 * M, ldb=2 * N)["path"] in ("planes128", "bf16x3")      # never the TN tile: M < 128
            assert _gemm_plan(1, 0, M, N, K, prec=0, **kw)["path"] == "f32"
    M, N, K, shifts = R.SHIFT_TN_CASE
    for s in shifts:
        assert _gemm_plan(1, 0, M, N, K, lda=2 * M, ldb=2 * N, shift=s)["path"] == "planes128"
        assert R.plan_tuple(_gemm_plan(1, 0, M, N, K - abs(s), lda=2 * M, ldb=2 * N)) == ("tn", (4, 2), 1, 2, R.NONE, R.NONE)
    # the first product of the pair: the plane path where it leaves A's planes behind, the TN tile in the last case (nothing to reuse)
    assert _gemm_plan(1, 0, 64, 64, 192, lda=128, ldb=128)["path"] == "planes128" and _gemm_plan(1, 0, M, N, K, lda=2 * M, ldb=2 * N)["path"] == "tn"


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, 2.0 - 3 * 2.0 ** -9, -3.0 - 2.0 ** -8, 7.013671875], np.float32)
    want = np.array([1.0, 1.0, 1.015625, 1.0078125, 1.9921875, -3.0, 7.0], np.float32)
    assert np.array_equal(R.bf16_round(x), want)
    import torch
    rs = np.random.RandomState(0)
    v = (rs.standard_normal(4096) * np.exp2(rs.uniform(-40, 40, 4096))).astype(np.float32)
    assert np.array_equal(R.bf16_round(v), torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy())
