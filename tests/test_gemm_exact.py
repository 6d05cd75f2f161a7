"""Every path of gemm.hip on the GPU, held to exact results on exactly summable operands (tests/gemm_ref.py: what the operands are, why their
product has no rounding in it, and the table of cases; tests/test_gemm_exact_host.py: the same claims checked on the CPU).

Per row of the table: the plan is asserted on the real device, then the product runs
  * on integers in [-7, 7] (both precisions, and gemm_bf16_single): np.array_equal with the float64 product;
  * on two-level operands p + q 2^-9 (precision 1): bit for bit  sum pa pb + 2^-9 sum (pa qb + qa pb)  (sum pa pb with gemm_bf16_single);
  * on scaled Gaussians: |C - C64| <= g (S + |beta C0|) per element with the derived g of gemm_ref.bound_g, and a second run with the rows
    of A and the columns of B scaled by powers of two must be the first result scaled, bit for bit.
Every run is poisoned: A, B and C are windows in NaN buffers (guard rows, row padding of 4 floats and of 1), the workspace is filled with 0xFF
bytes (bf16 NaNs) before each call, with beta = 0 the C window itself starts as NaN; afterwards the whole C buffer is compared as int32 --
the window with the expected bits, everything around it untouched.  Every run is made twice and must repeat its bits.

ctcn_gemm_shift_b and GemmPlanes::same_a run through ctcn_diag_gemm_shift_b_pair (the dW_ih / dW_hh pair of a recurrent layer): C2 = A^T
shift_k(B2) exactly, for both branches of split_transpose_tile, the queued split, the narrowed f32 window and the narrowed window on the TN tile;
The second product gets A's own device pointer, as in the layer.  C2 with the reuse request equals C2 without; that the planes really were
reused is shown on the device: the entry overwrites A with NaN between the two products (reuse = 2) and C2 must still be exact -- and must be
NaN where there is nothing to reuse (precision 0, a first product on the TN tile), which shows that the overwrite lands before the second
product reads.  A reuse request with another A (another buffer) is refused: C2 is that A's exact product, also with the first A overwritten.

Measured on an MI355X: all 81 rows and the 20 shifted / reused products exact.  Worst |C - C64| / bound of the generic family per path taken
(runs, worst ratio; each test prints its own):
    f32 56, 0.430 (K = 1: the bound is four roundings wide)   f32 split-K 4, 0.009     f32_queue 2, 0.136
    bf16x3 direct 40, 0.433                                    bf16x3 direct split-K 2, 0.025
    planes128 16, 0.318    planes128 split-K 5, 0.027          planes128_queue 4, 0.210
    planes256 9, 0.306     planes256_af32 3, 0.168             planes256_queue 2, 0.267
    tn (always split-K) 9, 0.027                               ctcn_gemm_dx 256 x 320 tile 2, 0.143
At K >= 64 the plane paths sit at 0.14-0.32 of the bound: with k rows of B spread over 2^20 one product carries S_ij, and its own split
error, up to 2^-16, is a third of g.  Where K is long and the terms comparable (the TN rows) the ratio is 0.03.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import gemm_ref as R
from test_host_logic import _gemm_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def workspace(dev, ws):
    """(tensor or None, pointer, bytes) of a case's workspace, every byte 0xFF."""
    from ctc_pytorch_amd import _lib
    _lib.status_word(dev)
    if ws is None:
        return None, None, 0
    w = _lib.workspace(dev) if ws == "main" else torch.empty(ws, dtype=torch.uint8, device=dev)
    w.fill_(0xFF)
    return w, ctypes.c_void_p(w.data_ptr()), w.numel()


def download(t):
    """The tensor on the host; a device fault ends the session there (nothing more is launched on a faulted device)."""
    try:
        return t.cpu().numpy()
    except RuntimeError as e:
        pytest.exit("device fault in test_gemm_exact, nothing more is launched: %s" % e, returncode=3)


def upload(buf, off, dev):
    t = torch.from_numpy(buf).to(dev)
    assert t.data_ptr() % 16 == 0
    return t, ctypes.c_void_p(t.data_ptr() + 4 * off)


def run_twice(case, dev, A, B, C0, pad, beta):
    """Two poisoned calls on the logical A (M x K) and B (K x N) framed at padding `pad`, each from a fresh C buffer and a workspace of 0xFF bytes.
    -> (C window, C buffer before, C buffer after, splits); the second call repeated the first one's bits, the operands are as they were."""
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    ta, tb, M, N, K = case["shape"]
    lda, ldb, ldc = R.leading_dims(case, pad)
    (Ab, aoff), (Bb, boff) = R.frame(R.stored(A, ta), lda), R.frame(R.stored(B, tb), ldb)
    (Ad, ap), (Bd, bp) = upload(Ab, aoff, dev), upload(Bb, boff, dev)
    before, coff = c_frame(C0, ldc, beta)
    prec, st, outs = case["prec"], _lib.stream_ptr(), []
    for _ in range(2):
        Cd, cp = upload(before, coff, dev)
        w, wp, wn = workspace(dev, case["ws"])
        # the plan on this device, with these pointers
        got = _gemm_plan(ta, tb, M, N, K, prec=prec, lda=lda, ldb=ldb, amod=ap.value % 16, bmod=bp.value % 16, xcd=case["xcd"],
                         ws=None if w is None else wn, cus=L.ctcn_device_cus(), xcds=L.ctcn_device_xcds())
        want = R.expected_plan(case, pad)
        assert (R.plan_tuple(got) if pad == 4 else (got["path"], got["splits"])) == want, (pad, got)
        if case["entry"] == "dx":
            out = (ctypes.c_int * 4)()
            assert L.ctcn_diag_dx_plan(M, N, K, lda, 1, ap.value % 16, 1, wn, L.ctcn_device_cus(), ctypes.cast(out, ctypes.c_void_p)) == 0
            assert (out[0], out[1]) == ((1, 1) if pad == 4 else (0, 0))
            rc = L.ctcn_gemm_dx(M, N, K, ap, lda, bp, ldb, cp, ldc, float(beta), prec, wp, wn, st)
        elif case["xcd"]:
            rc = L.ctcn_diag_gemm_on_xcds(ta, tb, M, N, K, ap, lda, bp, ldb, cp, ldc, float(beta), prec, wp, wn, st, case["xcd"])
        else:
            rc = L.ctcn_gemm(ta, tb, M, N, K, ap, lda, bp, ldb, cp, ldc, float(beta), prec, wp, wn, st)
        _lib.check(rc, "gemm")
        outs.append(download(Cd))
    assert np.array_equal(i32(download(Ad)), i32(Ab)) and np.array_equal(i32(download(Bd)), i32(Bb)), "an operand was written"
    after, again = outs
    assert np.array_equal(i32(after), i32(again)), "two runs differ"
    return R.window(after, coff, M, N, ldc), before, after, got["splits"]


def c_frame(C0, ldc, beta):
    """The C buffer before a call: C0 in the window (NaN when beta = 0: the kernel may not read it), NaN around it."""
    return R.frame(C0 if beta != 0.0 else np.full_like(C0, np.nan), ldc)


def assert_exact(case, dev, A, B, C0, prod, pad, beta, what):
    ta, tb, M, N, K = case["shape"]
    ldc = N + pad
    want, exact = R.with_beta(prod, C0, beta)
    assert exact
    got, before, after, _ = run_twice(case, dev, A, B, C0, pad, beta)
    expect, coff = R.frame(want, ldc)
    if not np.array_equal(i32(after), i32(expect)):
        bad = np.argwhere(i32(got) != i32(want))
        assert np.isfinite(got).all(), "%s pad %d beta %g: %d non-finite outputs, first at %s" % (what, pad, beta, (~np.isfinite(got)).sum(),
                                                                                               np.argwhere(~np.isfinite(got))[:1])
        assert len(bad) == 0, "%s pad %d beta %g: %d of %d outputs differ, first at %s: got %r want %r" % (
            what, pad, beta, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        raise AssertionError("%s pad %d beta %g: wrote outside the C window" % (what, pad, beta))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_every_path_is_exact_on_exactly_summable_operands(case, dev):
    ta, tb, M, N, K = case["shape"]
    rs = np.random.RandomState(zlib.crc32(case["id"].encode()) & 0x7FFFFFFF)
    fam = {}
    with R.set_options(case["opts"]):
        for name, pad, beta in R.combos(case):
            if name not in fam:
                if name == "int":
                    A, B = R.integers(rs, (M, K)), R.integers(rs, (K, N))
                    fam[name] = (A, B, R.c0_values(rs, (M, N)), R.expected_integers(A, B))
                elif name == "two":
                    (A, pa, qa), (B, pb, qb) = R.two_level(rs, (M, K), K), R.two_level(rs, (K, N), K)
                    fam[name] = (A, B, R.c0_values(rs, (M, N)), R.expected_two_level(pa, qa, pb, qb, single=case["single"]))
                else:
                    A, B, C0 = R.gaussian(rs, M, N, K)
                    fam[name] = (A, B, C0, R._mm(A, B), R._mm(np.abs(A), np.abs(B)), R.pow2_scales(rs, M, N))
            if name != "gauss":
                A, B, C0, prod = fam[name]
                assert_exact(case, dev, A, B, C0, prod, pad, beta, name)
                continue
            A, B, C0, C64, S, (sa, sb) = fam[name]
            ldc = N + pad
            got, before, after, splits = run_twice(case, dev, A, B, C0, pad, beta)
            got = got.copy()
            coff = R.GUARD * ldc
            R.window(after, coff, M, N, ldc)[...] = R.window(before, coff, M, N, ldc)
            assert np.array_equal(i32(after), i32(before)), "wrote outside the C window"
            assert np.isfinite(got).all()
            err = np.abs(got.astype(np.float64) - (C64 + beta * C0.astype(np.float64)))
            bound = R.bound_g(K, splits, case["prec"]) * (S + abs(beta) * np.abs(C0))
            ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size and K else 0.0
            print("gemm_exact ratio %s pad %d beta %g splits %d: worst error / bound %.4f" % (case["id"], pad, beta, splits, ratio))
            assert (err <= bound).all(), ratio
            got2 = run_twice(case, dev, A * sa, B * sb, C0 * sa * sb, pad, beta)[0]
            assert np.array_equal(i32(got2), i32(got * sa * sb)), "the scaled run is not the first run scaled"


# ---- ctcn_gemm_shift_b and plane reuse ------------------------------------------------------------------------------------------------
def pair(dev, M, N, K, A, A2, B1, B2, C0, prec, shift, beta, reuse, xcd, d, pad):
    """C1 = A^T B1, C2 = A2^T shift(B2): A stored K x M in column half d of a K x 2M NaN buffer, B1, B2 likewise in K x 2N.  A2 = None: the second
    product gets A's own device pointer, as in the layer; otherwise A2 is another buffer.  reuse: ctcn_diag_gemm_shift_b_pair's (2: A is
    overwritten with NaN between the products).  -> the two C windows, after checking that nothing outside them moved, that B1, B2 and A2 are as
    they were and that A is too (or, reuse = 2, that its window is NaN and nothing around it moved)."""
    from ctc_pytorch_amd import ops
    lda, ldb, ldc = 2 * M, 2 * N, N + pad
    fr = [R.frame(X, ld, col0=d * w) for X, ld, w in ((A, lda, M), (B1, ldb, N), (B2, ldb, N))] + ([R.frame(A2, lda, col0=d * M)] if A2 is not None else [])
    up = [upload(b, o, dev)[0] for b, o in fr]
    a, b1, b2 = (t[o:] for t, (_, o) in zip(up[:3], fr[:3]))
    a2 = up[3][fr[3][1]:] if A2 is not None else a
    assert (a2.data_ptr() == a.data_ptr()) == (A2 is None)
    cb = [c_frame(C0, ldc, beta) for _ in range(2)]
    cu = [upload(b.copy(), o, dev) for b, o in cb]
    w = workspace(dev, "main")[0]
    old = ops.get_precision()
    ops.set_precision(prec)
    try:
        ops.gemm_shift_b_pair(M, N, N, K, a, lda, b1, ldb, cu[0][0][cb[0][1]:], ldc, a2, b2, ldb, cu[1][0][cb[1][1]:], ldc, shift, beta=beta, xcd_allow=xcd,
                              reuse=reuse, ws=w)
    finally:
        ops.set_precision(old)
    outs = []
    for (before, off), (t, _) in zip(cb, cu):
        after = download(t)
        win = R.window(after, off, M, N, ldc).copy()
        R.window(after, off, M, N, ldc)[...] = R.window(before, off, M, N, ldc)
        assert np.array_equal(i32(after), i32(before)), "wrote outside the C window"
        outs.append(win)
    for j, ((before, off), t) in enumerate(zip(fr, up)):
        after = download(t)
        if j == 0 and reuse == 2:
            assert (i32(R.window(after, off, K, M, lda)) == -1).all(), "A was not overwritten between the products"
            R.window(after, off, K, M, lda)[...] = R.window(before, off, K, M, lda)
        assert np.array_equal(i32(after), i32(before)), "an operand was written"
    return outs


def two_level_expected(a, b):
    """Expected bf16x3 value of stored-K-major two-level operands, recovered from their own splits (hi = p, lo = q 2^-9: test_gemm_exact_host)."""
    ah, al = R.split_bf16(a)
    bh, bl = R.split_bf16(b)
    return R._mm(ah.T, bh.astype(np.float64) + bl) + R._mm(al.T, bh)


def check_pair(dev, M, N, K, shifts, family, prec, xcd=0, reused=True):
    """reused: the second product takes A's planes from the first (precision 1, both on the plane path).  Then a run that overwrites A with NaN
    between the products must still be exact -- the proof, on the device, that A was not split again; where nothing is reused (no planes at
    precision 0, a first product on the TN tile) the same run must give NaN, which shows that the overwrite lands before the second product."""
    rs = np.random.RandomState(zlib.crc32(("%s%d-%d-%d-%d-%d" % (family, prec, M, N, K, xcd)).encode()) & 0x7FFFFFFF)
    if family == "int":
        A, A2, B1, B2 = (R.integers(rs, (K, n)) for n in (M, M, N, N))
        expected = lambda a, b: R.expected_integers(a.T, b)
    else:
        A, A2, B1, B2 = (R.two_level(rs, (K, n), K)[0] for n in (M, M, N, N))
        expected = two_level_expected
    C0 = R.c0_values(rs, (M, N))
    for i, shift in enumerate(shifts):
        # shifts alternate in sign: beta, the column half and the padding move on other strides, so that each sign meets every one of them
        beta, d, pad = R.BETAS[(i + i // 2) % 4], (i // 2) % 2, (4, 1)[(i // 4) % 2]
        Bs = R.shift_rows(B2, shift)           # (a zero row shifted in has hi = lo = 0: it adds nothing)
        want1, e1 = R.with_beta(expected(A, B1), C0, beta)
        want2, e2 = R.with_beta(expected(A, Bs), C0, beta)
        want3, e3 = R.with_beta(expected(A2, Bs), C0, beta)
        assert e1 and e2 and e3
        what = (family, prec, M, N, K, shift, beta)
        run = lambda a2, reuse: pair(dev, M, N, K, A, a2, B1, B2, C0, prec, shift, beta, reuse, xcd, d, pad)
        c1, c2 = run(None, 0)
        assert np.array_equal(i32(c1), i32(want1)), what
        assert np.array_equal(i32(c2), i32(want2)), (what, int((i32(c2) != i32(want2)).sum()))
        r1, r2 = run(None, 1)
        assert np.array_equal(i32(r1), i32(c1)) and np.array_equal(i32(r2), i32(c2)), (what, "the reuse request changed the result")
        p1, p2 = run(None, 2)
        assert np.array_equal(i32(p1), i32(c1)), what
        if reused:
            assert np.array_equal(i32(p2), i32(c2)), (what, "the second product read A again: its planes were not reused")
        else:
            assert np.isnan(p2).all(), (what, "nothing to reuse here, yet the second product did not read A")
        o1, o2 = run(A2, 1)
        assert np.array_equal(i32(o1), i32(want1)) and np.array_equal(i32(o2), i32(want3)), (what, "stale planes of another A were reused")
        o1, o2 = run(A2, 2)                    # ... and with A gone: the refused request read A2, not A
        assert np.array_equal(i32(o1), i32(want1)) and np.array_equal(i32(o2), i32(want3)), (what, "stale planes of another A were reused")


@pytest.mark.parametrize("family,prec", [("int", 0), ("int", 1), ("two", 1)])
@pytest.mark.parametrize("M,N,K,shifts", R.SHIFT_CASES, ids=lambda v: str(v) if isinstance(v, int) else "s")
def test_shifted_b_and_plane_reuse_are_exact(dev, M, N, K, shifts, family, prec):
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    kw = dict(lda=2 * M, ldb=2 * N, cus=L.ctcn_device_cus(), xcds=L.ctcn_device_xcds(), ws=_lib.WORKSPACE_BYTES)
    for s in shifts:
        if prec == 1:
            assert R.plan_tuple(_gemm_plan(1, 0, M, N, K, shift=s, same_a=1, **kw)) == ("planes128", (2, 2), 0, 1, R.NONE, R.TR)
        else:
            assert _gemm_plan(1, 0, M, N, K - abs(s), prec=0, **kw)["path"] == "f32"
    check_pair(dev, M, N, K, shifts, family, prec, reused=prec == 1)


def test_shifted_b_on_the_side_stream_xcds(dev):
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    M, N, K = 64, 80, 200
    p = _gemm_plan(1, 0, M, N, K, lda=2 * M, ldb=2 * N, shift=-65, same_a=1, xcd=0xF0, cus=L.ctcn_device_cus(), xcds=L.ctcn_device_xcds(), ws=_lib.WORKSPACE_BYTES)
    assert R.plan_tuple(p) == ("planes128_queue", (2, 2), 0, 1, R.NONE, R.TRQ)
    for family in ("int", "two"):
        check_pair(dev, M, N, K, (1, -65, 64, -(K - 1)), family, 1, xcd=0xF0)


def test_shifted_b_narrowed_window_on_the_tn_tile(dev):
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    M, N, K, shifts = R.SHIFT_TN_CASE
    kw = dict(lda=2 * M, ldb=2 * N, cus=L.ctcn_device_cus(), xcds=L.ctcn_device_xcds(), ws=_lib.WORKSPACE_BYTES)
    for s in shifts:
        assert _gemm_plan(1, 0, M, N, K, shift=s, **kw)["path"] == "planes128"                   # the whole window would take the plane path,
        assert R.plan_tuple(_gemm_plan(1, 0, M, N, K - abs(s), **kw)) == ("tn", (4, 2), 1, 2, R.NONE, R.NONE)    # the narrowed one the TN tile
    for family in ("int", "two"):
        check_pair(dev, M, N, K, shifts, family, 1, reused=False)      # (the first product ran on the TN tile: no planes of A)
