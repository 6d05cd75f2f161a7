"""ctcn_gemm_dx on the GPU: the 256 x 320 float32-A tile (gemm_af32_n320pp_kernel) computes, bit for bit, what ctcn_gemm(0, 0, ...) computes
for the same product, and every call the tile cannot take is that call.

The tile adds, per accumulator and 16-k step in increasing k, al*bh, ah*bl, ah*bh on the split_bf16 planes -- the order of every plane tile
-- so the comparison is torch.equal, never a tolerance:
  * against ops.gemm(0, 0, ...) on the same operands where ctcn_diag_gemm_plan says that call takes a plane path in one K sweep.  (With
    split-K -- few tiles and K >= 1 024: the (256, 640, 2 560) case -- the plane path adds partial sums per K chunk, another order: there
    the direct call is held to the float64 tolerance only.)
  * in EVERY case against the 256 x 128 / 256 x 256 float32-A tile of the parent, which is what the layer's dx product ran on: an output row
    depends on its own row of A alone, so the operands repeated to >= 20 480 rows go to that tile (asserted from the plan) and its first M
    rows are the reference.
  * and against float64 with the tolerance of test_gpu_kernels.py::test_gemm: (4e-5 at precision 1) * 4 * max|A| max|B| sqrt(K) + 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANE_PATHS = (3, 4, 5, 6, 7)          # ctcn_diag_gemm_plan: planes 128-row tile, queued, 256-row tile, 256-row tile with float32 A, queued
AF32 = 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def gemm_plan(M, N, K, lda, ldb, ldc, prec, A):
    from ctc_pytorch_amd import _lib, ops
    L = _lib.lib()
    out = (ctypes.c_int * 12)()
    rc = L.ctcn_diag_gemm_plan(0, 0, M, N, K, lda, ldb, ldc, prec, 0, A.data_ptr() % 16, 0, 1, _lib.WORKSPACE_BYTES, 0, 0, 0, L.ctcn_device_cus(),
                               L.ctcn_device_xcds(), ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0
    return dict(path=out[0], splits=out[4])


def dx_plan(M, N, K, lda, prec, A):
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 4)()
    rc = L.ctcn_diag_dx_plan(M, N, K, lda, prec, A.data_ptr() % 16, 1, _lib.WORKSPACE_BYTES, L.ctcn_device_cus(), ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0
    return dict(eligible=out[0], wide=out[1])


def operands(M, N, K, lda, ldc, dev, seed):
    """Rows of A and of B scaled over 2^-10 .. 2^10: the lo planes carry bits that matter next to the hi planes of other rows."""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((M, lda)).astype(np.float32) * np.exp2(rs.uniform(-10, 10, (M, 1))).astype(np.float32)
    B = rs.standard_normal((K, N)).astype(np.float32) * np.exp2(rs.uniform(-10, 10, (K, 1))).astype(np.float32)
    C0 = rs.standard_normal((M, ldc)).astype(np.float32) * np.float32(np.abs(A).max() * np.abs(B).max())
    return A, B, C0, [torch.from_numpy(v).to(dev) for v in (A, B, C0)]


SHAPES = [(256, 320, 64),        # one tile, two stages
          (300, 640, 96),        # partial last M-tile, three stages: every stage(has1, has2) form
          (513, 640, 100),       # K tail, K % 32 != 0
          (257, 960, 160),       # tiles_n = 3: tile indexing past two
          (256, 640, 2560)]      # cfg2's K


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_wide_tile_equals_the_parent_tiles(dev, M, N, K, beta):
    from ctc_pytorch_amd import ops
    lda, ldc = K + 8, N + 4
    A, B, C0, (Ad, Bd, C0d) = operands(M, N, K, lda, ldc, dev, M + N + K)
    want = A[:, :K].astype(np.float64) @ B.astype(np.float64) + beta * C0[:, :N]
    tol = 4e-5 * 4 * float(np.abs(A[:, :K]).max() * np.abs(B).max()) * K ** 0.5 + 1e-6
    ops.set_precision(1)
    ops.set_option("gemm_dx_wide", 2)
    try:
        assert dx_plan(M, N, K, lda, 1, Ad) == dict(eligible=1, wide=1)
        C = C0d.clone()
        ops.gemm_dx(M, N, K, Ad, lda, Bd, N, C, ldc, beta=beta)
        got = C.cpu().numpy()
        err = float(np.abs(got[:, :N] - want).max())
        print("dx tile %s beta %g: max error %.3g of tolerance %.3g" % ((M, N, K), beta, err, tol))
        assert err < tol
        assert np.array_equal(got[:, N:], C0[:, N:]), "wrote outside the ldc window"
        # the direct call
        Cg = C0d.clone()
        ops.gemm(0, 0, M, N, K, Ad, lda, Bd, N, Cg, ldc, beta=beta)
        p = gemm_plan(M, N, K, lda, N, ldc, 1, Ad)
        if p["path"] in PLANE_PATHS and p["splits"] == 1:
            assert torch.equal(C, Cg)
        else:
            assert float(np.abs(Cg.cpu().numpy()[:, :N] - want).max()) < tol
        # the parent's float32-A tile: the same rows, repeated until the product is large enough for it
        reps = -(-20480 // M)
        Ar, Cr = Ad.repeat(reps, 1), C0d.repeat(reps, 1)
        assert gemm_plan(M * reps, N, K, lda, N, ldc, 1, Ar)["path"] == AF32
        ops.set_option("gemm_dx_wide", 0)
        ops.gemm_dx(M * reps, N, K, Ar, lda, Bd, N, Cr, ldc, beta=beta)
        assert torch.equal(Cr[:M], C) and torch.equal(Cr[-M:], C)
    finally:
        ops.set_option("gemm_dx_wide", 1)
        ops.set_precision(0)


@pytest.mark.parametrize("case", ["a_offset_4_bytes", "lda_odd", "n_636", "precision_0", "bf16_single", "option_0"])
def test_calls_the_tile_cannot_take_are_ctcn_gemm(dev, case):
    """Each condition of the tile's eligibility, one at a time, with the option at 2 (0 in the last case): the plan says `not wide`, and the result is
    ctcn_gemm(0, 0, ...)'s, bit for bit (the same launches), within the float64 tolerance of the precision."""
    from ctc_pytorch_amd import ops
    M, N, K = 300, (636 if case == "n_636" else 640), 96
    lda, ldc = (K + 1 if case == "lda_odd" else K + 8), N + 4
    prec = 0 if case == "precision_0" else 1
    A, B, C0, (Ad, Bd, C0d) = operands(M, N, K, lda, ldc, dev, 7)
    if case == "a_offset_4_bytes":
        flat = torch.empty(M * lda + 1, dtype=torch.float32, device=dev)
        flat[1:] = Ad.reshape(-1)
        Ad = flat[1:]
        assert Ad.data_ptr() % 16 == 4
    want = A[:, :K].astype(np.float64) @ B.astype(np.float64)
    tol = (2e-6 if prec == 0 else 4e-5) * 4 * float(np.abs(A[:, :K]).max() * np.abs(B).max()) * K ** 0.5 + 1e-6
    ops.set_precision(prec)
    ops.set_option("gemm_dx_wide", 0 if case == "option_0" else 2)
    ops.set_option("gemm_bf16_single", 1 if case == "bf16_single" else 0)
    try:
        p = dx_plan(M, N, K, lda, prec, Ad)
        assert p["wide"] == 0 and p["eligible"] == (1 if case == "option_0" else 0), p
        for beta in (0.0, 1.0):
            C, Cg = C0d.clone(), C0d.clone()
            ops.gemm_dx(M, N, K, Ad, lda, Bd, N, C, ldc, beta=beta)
            ops.gemm(0, 0, M, N, K, Ad, lda, Bd, N, Cg, ldc, beta=beta)
            assert torch.equal(C, Cg)
            assert float(np.abs(C.cpu().numpy()[:, :N] - (want + beta * C0[:, :N])).max()) < tol
            assert torch.equal(C[:, N:], C0d[:, N:])
    finally:
        ops.set_option("gemm_bf16_single", 0)
        ops.set_option("gemm_dx_wide", 1)
        ops.set_precision(0)


@pytest.mark.parametrize("T", [10, 320])
def test_lstm_layer_gradients_do_not_depend_on_the_tile(dev, T):
    """One bidirectional LSTM layer of cfg2's width (B = 32, I = 640, H = 320: dx = da[T*B x 2 560] W_ih[2 560 x 640]), forward + backward, with
    the tile off and forced: the output and the four weight gradients are bit-identical, and so is dx wherever the call with the tile off sums
    over K in one sweep (ctcn_diag_gemm_plan: a plane path without split-K) -- T = 320, where it runs on the 256 x 128 float32-A tile as at
    cfg2.  At T = 10 the 320-row product is split five ways over K when the tile is off (10 tiles on 256 CUs) and its partial sums are added
    in another order: the two dx are float32 sums of the same 3 x 2 560 bf16 products per element in two orders, so they differ by the
    rounding of the partial sums alone, at most 3 K 2^-24 = 4.6e-4 of the terms' magnitude; there dx is held to that as a rel-L2."""
    from ctc_pytorch_amd import ops
    B, I, H = 32, 640, 320
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, I, generator=g)
    dy = torch.randn(T, B, 2 * H, generator=g)
    ws = [torch.randn(4 * H, I, generator=g) * I ** -0.5, torch.randn(4 * H, H, generator=g) * H ** -0.5,
          torch.randn(4 * H, I, generator=g) * I ** -0.5, torch.randn(4 * H, H, generator=g) * H ** -0.5]
    runs = []
    ops.set_precision(1)
    try:
        for mode in (0, 2):
            ops.set_option("gemm_dx_wide", mode)
            xg = x.to(dev).requires_grad_(True)
            w = [v.to(dev).requires_grad_(True) for v in ws]
            if mode == 2:
                assert dx_plan(T * B, I, 8 * H, 8 * H, 1, xg) == dict(eligible=1, wide=1)
            y = ops.rnn_layer(xg, w[0], w[1], w[2], w[3], "lstm")
            y.backward(dy.to(dev))
            torch.cuda.synchronize()
            runs.append([y.detach(), xg.grad] + [p.grad for p in w])
        off = gemm_plan(T * B, I, 8 * H, 8 * H, I, I, 1, xg)
    finally:
        ops.set_option("gemm_dx_wide", 1)
        ops.set_precision(0)
    ops.check_health()
    assert all(torch.isfinite(t).all() for t in runs[1]) and float(runs[1][1].abs().max()) > 0
    assert (off["path"] == AF32 and off["splits"] == 1) if T == 320 else off["splits"] > 1, off
    for name, a, b in zip(("y", "dx", "dw_ih", "dw_hh", "dw_ih_reverse", "dw_hh_reverse"), runs[0], runs[1]):
        if name == "dx" and off["splits"] > 1:
            rel = float((a.double() - b.double()).norm() / b.double().norm())
            print("dx, tile off (split-K %d) against tile on: rel-L2 %.3g" % (off["splits"], rel))
            assert rel < 3 * 8 * H * 2.0 ** -24
        else:
            assert torch.equal(a, b), name
