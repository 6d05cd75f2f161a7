"""Parity tests of the HIP path (through the C ABI of libctcn.so) against the oracle and the golden vectors
captured from the reference.  All tests need the MI355X: run with `pytest -m gpu`.

Tolerances (SURVEY §8a "Parity tolerances", f32-exact MFMA mode): activations / log-probs max-abs <= 1e-5 ..
1e-4, CTC loss rel <= 1e-5, gradients rel-L2 <= 1e-4, arg-max / greedy / beam strings identical."""
import json
import os

import ctypes

import numpy as np
import pytest
import torch
import torch.nn as tnn

from oracle import np_ref as R
from oracle import beam_ref, torch_cpu
from ctc_pytorch_amd.testing import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return np.load(os.path.join(G, name + ".npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f32_strict_unless_stated():
    """Every test starts in precision 0 (exact f32 MFMA: the f32-strict gates of SURVEY 8a); tests that take a `prec`
    parameter switch to the bf16x3 mode themselves.  The library default (precision 1, ops.DEFAULT_PRECISION) is
    restored afterwards."""
    from ctc_pytorch_amd import ops
    ops.set_precision(0)
    yield
    ops.set_precision(ops.DEFAULT_PRECISION)


# SURVEY 8a gates of the bf16-operand mode (precision 1 = bf16x3 split operands, ~2^-16 per product): activations / log-probs
# max-abs <= 1e-3, loss rel <= 1e-3, gradients and parameters after 3 Adam steps rel-L2 <= 1e-3, arg-max identical.
def gates(prec, strict_act, strict_grad, strict_loss):
    return (strict_act, strict_grad, strict_loss) if prec == 0 else (1e-3, 1e-3, 1e-3)


def argmax_report(lp, want, what):
    """arg-max must be identical; when it is not, say how close the flipped frames' top-2 margins are."""
    from ctc_pytorch_amd import ops
    got = ops.argmax_last(lp).cpu().numpy()
    want = np.asarray(want).astype(np.int32)
    if np.array_equal(got, want):
        return
    v = lp.detach().cpu().numpy()
    bad = np.argwhere(got != want)
    top2 = np.sort(v[tuple(bad.T)], axis=-1)[:, -2:]
    raise AssertionError("%s: %d arg-max flips; top-2 margins of the flipped frames: %s" % (what, len(bad), (top2[:, 1] - top2[:, 0])[:8]))


def gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def maxabs(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0


def rel_l2(a, b):
    a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---------------------------------------------------------------------------------------------------------
def test_library_loaded_is_in_tree():
    from ctc_pytorch_amd import _lib
    assert _lib.SO_PATH.endswith(os.path.join("ctc_pytorch_amd", "libctcn.so")) and os.path.exists(_lib.SO_PATH)
    assert _lib.lib().ctcn_version() >= 100
    assert _lib.lib().ctcn_device_cus() > 0


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 62, 40), (62, 640, 6400), (1280, 40, 512), (33, 17, 5), (300, 257, 130)])
def test_gemm(dev, ta, tb, M, N, K, prec):
    """precision 0: exact f32 MFMA; precision 1: bf16x3 split-operand MFMA (relative error ~2^-16 per product)."""
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    rs = np.random.RandomState(M * 7 + N * 3 + K + ta * 2 + tb)
    A = rs.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    Bm = rs.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    C0 = rs.standard_normal((M, N + 3)).astype(np.float32)
    want = (A.T if ta else A).astype(np.float64) @ (Bm.T if tb else Bm).astype(np.float64)
    for beta in (0.0, 1.0):
        C = gpu(C0, dev)
        ops.gemm(ta, tb, M, N, K, gpu(A, dev), A.shape[1], gpu(Bm, dev), Bm.shape[1], C, N + 3, beta=beta)
        got = C.cpu().numpy()
        ref = want + beta * C0[:, :N]
        scale = np.abs(A).max() * np.abs(Bm).max() * np.sqrt(K)
        tol = (2e-6 if prec == 0 else 4e-5) * scale * 4 + 1e-6
        err = np.max(np.abs(got[:, :N] - ref))
        if not (err < tol and np.array_equal(got[:, N:], C0[:, N:])):
            ops.set_precision(0)
        assert err < tol, (ta, tb, M, N, K, beta, err, tol)
        assert np.array_equal(got[:, N:], C0[:, N:]), "wrote outside ldc window"
    ops.set_precision(0)


@pytest.mark.parametrize("M,N,K,pad", [(1280, 640, 25600, 0), (1280, 320, 25568, 0), (388, 132, 1100, 8), (1536, 512, 4099, 4), (960, 320, 9600, 0),
                                         (128, 64, 1024, 0), (2048, 2560, 2048, 0), (4096, 4100, 1056, 4)])
def test_gemm_tn_tile(dev, M, N, K, pad):
    """precision 1, C = A^T B with both operands contraction-major (the weight gradients): the TN tile (`gemm_tn`, float32 rows split
    while they are staged, ds_read_b64_tr_b16 fragments, split-K queue) against float64, against the plane path (same bf16x3 operands
    and products, only the order of the k-sums differs), with ragged M / N / K, padded leading dimensions and beta = 1 (the last shape has
    so many tiles that it runs without split-K: beta is applied in the tile's own epilogue); a second run is bit-identical (the split-K partials are reduced in a fixed order whichever workgroup made them)."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(M + N + K)
    A = torch.from_numpy(rs.standard_normal((K, M + pad)).astype(np.float32)).to(dev)
    B = torch.from_numpy(rs.standard_normal((K, N + pad)).astype(np.float32)).to(dev)
    C0 = torch.from_numpy(rs.standard_normal((M, N + 3)).astype(np.float32)).to(dev)
    ref = A[:, :M].double().t() @ B[:, :N].double()
    ops.set_precision(1)
    try:
        for beta in (0.0, 1.0):
            outs = []
            for tn in (1, 1, 0):
                ops.set_option("gemm_tn", tn)
                C = C0.clone()
                ops.gemm(1, 0, M, N, K, A, M + pad, B, N + pad, C, N + 3, beta=beta)
                outs.append(C)
            want = ref + beta * C0[:, :N].double()
            tol = 4e-5 * 4 * float(A.abs().max() * B.abs().max()) * K ** 0.5
            for o in outs:
                assert float((o[:, :N].double() - want).abs().max()) < tol
                assert torch.equal(o[:, N:], C0[:, N:]), "wrote outside the ldc window"
            assert torch.equal(outs[0], outs[1])
            assert float((outs[0][:, :N] - outs[2][:, :N]).abs().max()) < 1e-5 * K ** 0.5
    finally:
        ops.set_option("gemm_tn", 1)
        ops.set_precision(0)


@pytest.mark.parametrize("M,N,K,ta,tb", [(8192, 1024, 200, 0, 1), (1024, 8192, 136, 0, 1), (8190, 1030, 72, 0, 0), (25600, 640, 1280, 0, 0)])
def test_gemm_bf16x3_big_tiles_equal_small_tiles(dev, M, N, K, ta, tb):
    """precision 1: the optional 256x128 / 128x256 workgroup tiles (`gemm_big_tiles`; fewer LDS fragment reads per MFMA,
    but one workgroup per CU: measured slower, so off by default) accumulate every output element over k in the same
    order with the same operands as the 128x128 tiling: bit-identical results, both within bf16x3 accuracy of float64."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(M % 1000 + K)
    A = torch.from_numpy(rs.standard_normal((K, M) if ta else (M, K)).astype(np.float32)).to(dev)
    B = torch.from_numpy(rs.standard_normal((N, K) if tb else (K, N)).astype(np.float32)).to(dev)
    outs = []
    ops.set_precision(1)
    try:
        for big in (0, 1):
            ops.set_option("gemm_big_tiles", big)
            C = torch.full((M, N), float("nan"), device=dev)
            ops.gemm(ta, tb, M, N, K, A, A.shape[1], B, B.shape[1], C, N)
            outs.append(C)
    finally:
        ops.set_option("gemm_big_tiles", 0)
        ops.set_precision(0)
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1])
    rows = torch.arange(0, M, max(1, M // 64), device=dev)
    Ad = (A.t() if ta else A)[rows].double()
    ref = Ad @ (B.t() if tb else B).double()
    assert float((outs[1][rows].double() - ref).abs().max()) < 2e-4 * (K ** 0.5)


@pytest.mark.parametrize("M,N,K,ta,tb,beta", [(25600, 1280, 640, 0, 1, 0.0), (25600, 640, 2560, 0, 0, 0.0), (16390, 1030, 200, 0, 1, 1.0),
                                                  (8192, 2560, 136, 0, 1, 0.0), (12800, 96, 320, 0, 0, 1.0), (76800, 1536, 1024, 0, 1, 0.0),
                                                  # the float32-A tile (A split while it is staged) with a K tail inside its last stage, ragged M: 256 x 128 and 256 x 256
                                                  (16390, 384, 1300, 0, 1, 1.0), (25001, 512, 204, 0, 0, 0.0), (25600, 640, 36, 0, 1, 0.0)])
def test_gemm_bf16x3_tile256_equals_tile128(dev, M, N, K, ta, tb, beta):
    """precision 1: the 256 x 256 / 256 x 128 workgroup tiles (global_load_lds staging, `gemm_tile256`, the default for
    activation-sized products) accumulate every output element over k in the same order with the same operands as the
    128 x 128 tiling: bit-identical results (ragged M / N / K edges and beta = 1 included), within bf16x3 accuracy of float64."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(M % 1000 + K)
    A = torch.from_numpy(rs.standard_normal((K, M) if ta else (M, K)).astype(np.float32)).to(dev)
    B = torch.from_numpy(rs.standard_normal((N, K) if tb else (K, N)).astype(np.float32)).to(dev)
    C0 = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(dev)
    outs = []
    ops.set_precision(1)
    try:
        for t256, inline in ((0, 0), (1, 0), (1, 1)):
            ops.set_option("gemm_tile256", t256)
            ops.set_option("gemm_a_inline", inline)        # A split into planes while it is staged (row-major A only)
            C = C0.clone()
            ops.gemm(ta, tb, M, N, K, A, A.shape[1], B, B.shape[1], C, N, beta=beta)
            outs.append(C)
    finally:
        ops.set_option("gemm_tile256", 1)
        ops.set_option("gemm_a_inline", 1)
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    rows = torch.arange(0, M, max(1, M // 64), device=dev)
    ref = (A.t() if ta else A)[rows].double() @ (B.t() if tb else B).double() + beta * C0[rows].double()
    assert float((outs[1][rows].double() - ref).abs().max()) < 2e-4 * (K ** 0.5)


@pytest.mark.parametrize("ta,tb,M,N,K,beta", [(0, 1, 8192, 1536, 136, 0.0), (0, 1, 25600, 2560, 640, 1.0),          # plane tile 256 x 256
                                                  (0, 1, 16390, 1664, 200, 1.0),                                        # plane tile 256 x 128, ragged
                                                  (0, 0, 25600, 640, 2560, 0.0), (0, 0, 25001, 512, 204, 1.0),          # float32-A tile, K tail, ragged M
                                                  (0, 1, 16390, 384, 1300, 1.0),                                        # float32-A tile 256 x 128
                                                  (1, 0, 1280, 640, 25600, 0.0), (1, 0, 1280, 320, 25568, 1.0),         # TN tile, split-K
                                                  (1, 0, 644, 132, 5000, 1.0), (1, 0, 4096, 4100, 1056, 1.0)])          # TN tile ragged / without split-K
def test_gemm_bf16_single_is_the_product_of_the_rounded_operands(dev, ta, tb, M, N, K, beta):
    """Option "gemm_bf16_single" on the three 256-row tiles: C = bf16(A) bf16(B) with f32 accumulation -- against the float64 product of the
    bf16-rounded operands (only the f32 summation differs: 2e-5 of the result's scale), which is NOT the bf16x3 result of the default mode (the
    mode did switch tiles); beta = 1 and the columns outside the ldc window as in the other tile tests; a second run is bit-identical."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(M % 1000 + K + N)
    A = torch.from_numpy(rs.standard_normal((K, M) if ta else (M, K)).astype(np.float32)).to(dev)
    B = torch.from_numpy(rs.standard_normal((N, K) if tb else (K, N)).astype(np.float32)).to(dev)
    C0 = torch.from_numpy(rs.standard_normal((M, N + 4)).astype(np.float32)).to(dev)
    outs = []
    ops.set_precision(1)
    try:
        for single in (0, 1, 1):
            ops.set_option("gemm_bf16_single", single)
            C = C0.clone()
            ops.gemm(ta, tb, M, N, K, A, A.shape[1], B, B.shape[1], C, N + 4, beta=beta)
            outs.append(C)
    finally:
        ops.set_option("gemm_bf16_single", 0)
        ops.set_precision(0)
    rows = torch.arange(0, M, max(1, M // 96), device=dev)
    Ar, Br = (A.t() if ta else A)[rows], (B.t() if tb else B)
    exact = Ar.double() @ Br.double() + beta * C0[rows, :N].double()
    rounded = Ar.bfloat16().double() @ Br.bfloat16().double() + beta * C0[rows, :N].double()
    scale = K ** 0.5
    assert torch.equal(outs[1], outs[2])
    assert torch.equal(outs[1][:, N:], C0[:, N:]), "wrote outside the ldc window"
    assert float((outs[1][rows, :N].double() - rounded).abs().max()) < 2e-5 * scale
    assert float((outs[0][rows, :N].double() - exact).abs().max()) < 2e-4 * scale
    assert float((outs[1][rows, :N].double() - exact).abs().max()) > 1e-3 * scale          # bf16 operands: the third digit moves


def test_gemm_side_stream_forms_equal_the_whole_device_forms(dev):
    """ops.gemm(..., xcd_allow=mask) = ctcn_diag_gemm_on_xcds: the queued forms a side stream next to a persistent recurrence runs (workgroups
    off the XCDs of `mask` exit, the others pull tiles from an atomic queue) -- gemm_f32_queue_kernel, gemm_planes_nt_queue_kernel (+
    split_transpose_queue_kernel for a contraction-major operand), gemm_planes_nt256pp_queue_kernel and the TN tile with an XCD mask --
    against mask 0, bit for bit (the same tile code; the plane tiles are bit-identical across tile sizes by design, and the TN partials are
    summed in split order: tn_splits_force = 2 gives every mask the same two k windows), with beta = 0 and 1 and columns beyond N that must
    stay untouched.  The plan of every call is asserted first, so that a rule that moved cannot turn the test into mask 0 against mask 0."""
    from ctc_pytorch_amd import ops, _lib
    from test_host_logic import _gemm_plan
    L = _lib.lib()
    cus, xcds = L.ctcn_device_cus(), L.ctcn_device_xcds()
    if xcds < 8:
        pytest.skip("needs a device of 8 XCDs (masks 0x01 and 0xF0)")
    cases = [   # prec, ta, tb, M, N, K, options, {mask: path}
        (0, 0, 0, 200, 62, 40, {}, {0: "f32", 0x01: "f32_queue", 0xF0: "f32_queue"}),
        (1, 0, 0, 300, 257, 130, {}, {0: "planes128", 0x01: "planes128_queue", 0xF0: "planes128_queue"}),
        (1, 0, 1, 300, 257, 130, {}, {0: "planes128", 0x01: "planes128_queue", 0xF0: "planes128_queue"}),
        (1, 1, 1, 300, 257, 130, {}, {0: "planes128", 0x01: "planes128_queue", 0xF0: "planes128_queue"}),
        (1, 0, 1, 6144, 128, 64, {}, {0: "planes128", 0x01: "planes256_queue", 0xF0: "planes128_queue"}),
        (1, 1, 0, 388, 132, 1100, {"tn_splits_force": 2}, {0: "tn", 0x01: "tn", 0xF0: "tn"}),
        (1, 1, 0, 128, 64, 1024, {"tn_splits_force": 2}, {0: "tn", 0x01: "tn", 0xF0: "tn"}),
    ]
    try:
        for prec, ta, tb, M, N, K, opts, paths in cases:
            ops.set_precision(prec)
            for n, v in opts.items():
                ops.set_option(n, v)
            rs = np.random.RandomState(M + 3 * N + K + ta * 2 + tb)
            A = gpu(rs.standard_normal((K, M) if ta else (M, K)).astype(np.float32), dev)
            Bm = gpu(rs.standard_normal((N, K) if tb else (K, N)).astype(np.float32), dev)
            C0 = gpu(rs.standard_normal((M, N + 3)).astype(np.float32), dev)
            ref = (A.t() if ta else A).double() @ (Bm.t() if tb else Bm).double()
            for mask, path in paths.items():
                got = _gemm_plan(ta, tb, M, N, K, prec=prec, amod=A.data_ptr() % 16, bmod=Bm.data_ptr() % 16, xcd=mask, cus=cus, xcds=xcds)
                assert got["path"] == path and (path != "tn" or got["splits"] == 2), (M, N, K, mask, got)
            for beta in (0.0, 1.0):
                outs = {}
                for mask in paths:
                    C = C0.clone()
                    ops.gemm(ta, tb, M, N, K, A, A.shape[1], Bm, Bm.shape[1], C, N + 3, beta=beta, xcd_allow=mask)
                    outs[mask] = C
                tol = (2e-6 if prec == 0 else 4e-5) * 4 * float(A.abs().max() * Bm.abs().max()) * K ** 0.5 + 1e-6
                assert float((outs[0][:, :N].double() - (ref + beta * C0[:, :N].double())).abs().max()) < tol
                for mask in (0x01, 0xF0):
                    assert torch.equal(outs[mask], outs[0]), (prec, ta, tb, M, N, K, beta, mask)
                    assert torch.equal(outs[mask][:, N:], C0[:, N:]), "wrote outside the ldc window"
            for n in opts:
                ops.set_option(n, 0)
    finally:
        ops.set_option("tn_splits_force", 0)
        ops.set_precision(0)


@pytest.mark.parametrize("kind", ["lstm", "gru", "rnn"])
def test_rnn_layer_golden(dev, kind):
    from ctc_pytorch_amd import ops
    z = load("rnn_" + kind)
    x = gpu(z["x"], dev).requires_grad_(True)
    names = ["weight_ih_l0", "weight_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse"]
    w = [gpu(z["w.rnn." + n], dev).requires_grad_(True) for n in names]
    y = ops.rnn_layer(x, w[0], w[1], w[2], w[3], {"rnn": "tanh"}.get(kind, kind))
    assert maxabs(y, z["y"]) < 5e-6
    y.backward(gpu(z["dy"], dev))
    assert maxabs(x.grad, z["dx"]) < 2e-5
    for n, p in zip(names, w):
        assert maxabs(p.grad, z["g.rnn." + n]) < 1e-4, n


@pytest.mark.parametrize("kind,T,B,I,H,bi", [("lstm", 37, 32, 40, 320, True), ("gru", 19, 64, 48, 512, True),
                                            ("lstm", 11, 70, 24, 128, True), ("rnn", 23, 5, 12, 36, False),
                                            ("gru", 9, 3, 20, 24, True), ("lstm", 6, 16, 640, 20, False),
                                            ("lstm", 1, 4, 8, 16, True), ("gru", 2, 1, 8, 8, True), ("lstm", 7, 17, 12, 1024, False),
                                            ("lstm", 5, 200, 16, 64, True), ("rnn", 3, 33, 4, 512, True), ("gru", 12, 130, 8, 40, True)])
def test_rnn_layer_vs_torch_cpu(dev, kind, T, B, I, H, bi):
    from ctc_pytorch_amd import ops
    cls = {"lstm": tnn.LSTM, "gru": tnn.GRU, "rnn": tnn.RNN}[kind]
    torch.manual_seed(T * 100 + B)
    ref = cls(I, H, bidirectional=bi, bias=False)
    x = torch.randn(T, B, I)
    dy = torch.randn(T, B, (2 if bi else 1) * H)
    xr = x.clone().requires_grad_(True)
    yr, _ = ref(xr)
    yr.backward(dy)
    names = ["weight_ih_l0", "weight_hh_l0"] + (["weight_ih_l0_reverse", "weight_hh_l0_reverse"] if bi else [])
    w = [getattr(ref, n).detach().to(dev).requires_grad_(True) for n in names] + ([None, None] if not bi else [])
    xg = x.to(dev).requires_grad_(True)
    y = ops.rnn_layer(xg, w[0], w[1], w[2], w[3], {"rnn": "tanh"}.get(kind, kind))
    assert maxabs(y, yr) < 2e-5
    y.backward(dy.to(dev))
    assert rel_l2(xg.grad, xr.grad) < 1e-4
    for n, p in zip(names, w):
        assert rel_l2(p.grad, getattr(ref, n).grad) < 1e-4, n


@pytest.mark.parametrize("kind,T,B,I,H,bi", [("lstm", 120, 32, 40, 320, True), ("gru", 40, 64, 48, 512, True), ("lstm", 33, 70, 24, 128, True),
                                            ("rnn", 50, 5, 12, 36, False), ("gru", 30, 3, 20, 24, True), ("lstm", 20, 16, 64, 20, False),
                                            ("lstm", 1, 4, 8, 16, True), ("gru", 2, 1, 8, 8, True), ("lstm", 7, 17, 12, 1024, False),
                                            ("lstm", 5, 200, 16, 64, True), ("rnn", 9, 33, 4, 512, True), ("gru", 12, 130, 8, 40, True)])
def test_rnn_layer_bf16x3_vs_torch_cpu(dev, kind, T, B, I, H, bi):
    """precision=1: input projection AND the recurrent matmul run as bf16x3 split-operand MFMA (hi/lo planes handed
    between workgroups); outputs within 1e-4, gradients within 5e-4 rel-L2 of the f32 torch CPU layer (north-star
    gate 1e-3)."""
    from ctc_pytorch_amd import ops
    cls = {"lstm": tnn.LSTM, "gru": tnn.GRU, "rnn": tnn.RNN}[kind]
    torch.manual_seed(T * 100 + B + 7)
    ref = cls(I, H, bidirectional=bi, bias=False)
    x = torch.randn(T, B, I)
    dy = torch.randn(T, B, (2 if bi else 1) * H)
    xr = x.clone().requires_grad_(True)
    yr, _ = ref(xr)
    yr.backward(dy)
    names = ["weight_ih_l0", "weight_hh_l0"] + (["weight_ih_l0_reverse", "weight_hh_l0_reverse"] if bi else [])
    w = [getattr(ref, n).detach().to(dev).requires_grad_(True) for n in names] + ([None, None] if not bi else [])
    xg = x.to(dev).requires_grad_(True)
    ops.set_precision(1)
    try:
        y = ops.rnn_layer(xg, w[0], w[1], w[2], w[3], {"rnn": "tanh"}.get(kind, kind))
        y.backward(dy.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_precision(0)
    ops.check_health()
    assert maxabs(y, yr) < 1e-4
    assert rel_l2(xg.grad, xr.grad) < 5e-4
    for n, p in zip(names, w):
        assert rel_l2(p.grad, getattr(ref, n).grad) < 5e-4, n


@pytest.mark.parametrize("kind,T,B,I,H,bi", [("lstm", 60, 32, 40, 320, True), ("gru", 25, 9, 16, 128, True), ("rnn", 31, 20, 8, 48, False),
                                            ("lstm", 17, 70, 12, 64, True), ("gru", 12, 64, 24, 512, True)])
def test_rnn_persistent_equals_per_step_launches(dev, kind, T, B, I, H, bi):
    """The persistent recurrence (in-launch granule hand-off) and the one-launch-per-timestep path agree."""
    from ctc_pytorch_amd import ops
    G = {"lstm": 4, "gru": 3, "rnn": 1}[kind]
    torch.manual_seed(7)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    outs, grads = [], []
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    try:
        for flag in (0, 1):
            ops.set_rnn_persistent(flag)
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], {"rnn": "tanh"}.get(kind, kind))
            y.backward(dy)
            outs.append(y.detach().clone())
            grads.append([xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None])
            ops.check_health(dev)
    finally:
        ops.set_rnn_persistent(1)
    assert torch.isfinite(outs[1]).all()
    assert maxabs(outs[0], outs[1]) < 2e-6
    for g0, g1 in zip(grads[0], grads[1]):
        assert torch.isfinite(g1).all()
        assert rel_l2(g1, g0) < 2e-6


@pytest.mark.parametrize("kind,T,B,I,H,bi", [("lstm", 40, 144, 48, 320, True), ("gru", 33, 300, 24, 256, True), ("lstm", 25, 288, 16, 320, False), ("lstm", 30, 140, 40, 512, True)])
def test_rnn_batch_chunks_equal_one_launch_per_timestep(dev, kind, T, B, I, H, bi):
    """A batch that no persistent launch holds runs as batch chunks of ops.persistent_batch_limit rows, one persistent launch each (round 4),
    from the shape's second call on -- the first call is seen to fall back to the per-timestep kernels and marks the shape.  Output, input
    gradient and weight gradients agree with the unchunked layer (the per-timestep kernels) to the rounding the two kernel families differ by;
    the layer's dropout is the separate pass over the concatenated output (same mask as layer-then-dropout, bit for bit)."""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    G = {"lstm": 4, "gru": 3}[kind]
    torch.manual_seed(3)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    key = ({"lstm": 0, "gru": 1}[kind], H, 2 if bi else 1, B)
    ops._fallback_shapes.discard(key)
    runs = {}
    try:
        for mode in ("first", "chunks", "chunks_drop", "whole"):
            ops.set_batch_chunks(mode != "whole")
            ops._drop_counter[0] = 77
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], kind, True, 0.3 if mode == "chunks_drop" else 0.0)
            y.backward(dy)
            torch.cuda.synchronize()
            ops.check_health(dev)
            runs[mode] = (y.detach().clone(), [xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None], ops.rnn_last_kernels())
            if mode == "first" and key not in ops._fallback_shapes:
                pytest.skip("this shape runs persistently in one launch on this device: %s" % (runs[mode][2],))
    finally:
        ops.set_batch_chunks(True)
        ops._fallback_shapes.discard(key)
    assert "step" in runs["first"][2][0] + runs["first"][2][1] and "step" not in runs["chunks"][2][0] + runs["chunks"][2][1], (runs["first"][2], runs["chunks"][2])
    assert "step" in runs["whole"][2][0] + runs["whole"][2][1]
    assert maxabs(runs["whole"][0], runs["chunks"][0]) < 5e-5
    for g0, g1 in zip(runs["whole"][1], runs["chunks"][1]):
        assert torch.isfinite(g1).all() and rel_l2(g1, g0) < 5e-5
    ops._drop_counter[0] = 77
    assert torch.equal(runs["chunks_drop"][0], ops.dropout(runs["chunks"][0], 0.3, True))


@pytest.mark.parametrize("B,H", [(160, 320), (144, 512)])
def test_rnn_batch_chunks_into_flat_gradients(dev, B, H):
    """ Batch chunks whose weight gradients ACCUMULATE into shared flat-gradient views (the FlatAdam arrangement, `_ctcn_grad`)
    with the side stream forced on for every size: all chunks of a layer must write those views on the main stream, in order (a 32-row
    chunk at H = 320 has idle XCDs and would otherwise defer its GEMMs to the side stream, next to a sibling chunk's inline
    read-modify-write of the same buffers).  Two stacked layers, so that a recurrence follows and the deferral path is live; three
    repetitions must give bit-identical gradients, and they must agree with the unchunked per-timestep kernels."""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    T, I = 30, 48
    torch.manual_seed(5)
    x = torch.randn(T, B, I, device=dev)
    mk = lambda i: [torch.randn(4 * H, i, device=dev) * 0.1, torch.randn(4 * H, H, device=dev) * (1.0 / H ** 0.5),
                    torch.randn(4 * H, i, device=dev) * 0.1, torch.randn(4 * H, H, device=dev) * (1.0 / H ** 0.5)]
    w0, w1 = mk(I), mk(2 * H)
    dy = torch.randn(T, B, 2 * H, device=dev)
    key = (0, H, 2, B)

    def run(chunks, flat):
        ops.set_batch_chunks(chunks)
        ws = [t.clone().requires_grad_(True) for t in w0 + w1]
        views = None
        if flat:
            views = [torch.zeros_like(t) for t in ws]
            for t, g in zip(ws, views):
                t._ctcn_grad = g
        xs = x.clone().requires_grad_(True)
        h = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], "lstm", True, 0.0)
        y = ops.rnn_layer(h, ws[4], ws[5], ws[6], ws[7], "lstm", True, 0.0)
        y.backward(dy)
        ops.join_side_stream()
        torch.cuda.synchronize()
        ops.check_health(dev)
        return [xs.grad.clone()] + ([g.clone() for g in views] if flat else [t.grad.clone() for t in ws]), ops.rnn_last_kernels()

    ops._fallback_shapes.discard(key)
    try:
        ops.set_side_stream(True, 0)
        ref, names_ref = run(False, False)                 # unchunked: the per-timestep kernels
        assert "step" in names_ref[0] + names_ref[1], names_ref
        ops.mark_batch_chunks("lstm", H, 2, B)
        got = [run(True, True) for _ in range(3)]
    finally:
        ops.set_side_stream(True, ops.SIDE_MIN_ITEMS_FWD, ops.SIDE_MIN_ITEMS_BWD)
        ops.set_batch_chunks(True)
        ops._fallback_shapes.discard(key)
    assert "step" not in got[0][1][0] + got[0][1][1], got[0][1]
    for rep in got[1:]:
        for a, b in zip(got[0][0], rep[0]):
            assert torch.equal(a, b), "chunked weight gradients differ between repetitions (a race on the shared views)"
    for g1, g0 in zip(got[0][0], ref):
        assert torch.isfinite(g1).all() and rel_l2(g1, g0) < 5e-5


@pytest.mark.parametrize("kind,T,B,I,H,bi,drop", [("lstm", 50, 32, 40, 320, True, 0.0), ("lstm", 40, 8, 64, 384, True, 0.2), ("gru", 30, 64, 24, 512, True, 0.0),
                                                 ("lstm", 21, 9, 16, 640, True, 0.1), ("rnn", 31, 20, 8, 48, False, 0.0), ("gru", 25, 9, 16, 128, True, 0.3),
                                                 ("lstm", 19, 33, 12, 448, False, 0.0), ("lstm", 23, 16, 32, 72, True, 0.0)])
def test_rnn_bwd_item_gather_equals_scatter(dev, kind, T, B, I, H, bi, drop):
    """rnn_bwd_scatter2 (round 3: item-wave gather, one barrier per step, reserve traffic through LDS DMA) against the other backward kernels
    of precision 1 on the same layer: every cell type, 5 .. 40 slices (H = 72 .. 640; H = 640 has no other persistent kernel: the reference
    is the per-timestep path), partial batch tiles, one direction, padded last slice (H = 72), and the layer dropout applied by the
    recurrence.  Same products, the sum over sources grouped differently: gradients agree to float32 rounding of those sums."""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    G = {"lstm": 4, "gru": 3, "rnn": 1}[kind]
    torch.manual_seed(11)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    runs = {}
    try:
        for mode in ("reference", "item_gather"):
            ops.set_option("bwd_item_gather", 2 if mode == "item_gather" else 0)
            if mode == "reference" and H > 512:
                ops.set_rnn_persistent(0)
            ops._drop_counter[0] = 0
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], {"rnn": "tanh"}.get(kind, kind), True, drop)
            y.backward(dy)
            torch.cuda.synchronize()
            ops.check_health(dev)
            runs[mode] = (y.detach().clone(), [xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None], ops.rnn_last_kernels()[1])
            ops.set_rnn_persistent(1)
    finally:
        ops.set_option("bwd_item_gather", 1)
        ops.set_rnn_persistent(1)
    assert runs["item_gather"][2] == "rnn_bwd_scatter2", runs["item_gather"][2]
    assert runs["reference"][2] in ("rnn_bwd_scatter", "rnn_bwd_persist", "rnn_bwd_step")
    if H <= 512:
        assert torch.equal(runs["reference"][0], runs["item_gather"][0])              # same forward kernel: identical outputs (and dropout masks)
    for g0, g1 in zip(runs["reference"][1], runs["item_gather"][1]):
        assert torch.isfinite(g1).all()
        assert rel_l2(g1, g0) < 5e-6, rel_l2(g1, g0)


@pytest.mark.parametrize("kind,T,B,I,H,bi,prec", [("gru", 40, 64, 24, 512, True, 1), ("lstm", 30, 64, 16, 512, True, 1), ("lstm", 50, 32, 40, 320, True, 1),
                                                 ("lstm", 25, 128, 12, 128, True, 1), ("gru", 20, 64, 16, 256, True, 0), ("lstm", 33, 40, 16, 384, False, 1)])
def test_rnn_results_do_not_depend_on_the_xcd_order(dev, kind, T, B, I, H, bi, prec):
    """ADVICE r5 / VERDICT r5 weak 1: option "xcd_interleave" decides which PHYSICAL XCD hosts group g of a persistent recurrence -- a
    relabelling.  Outputs, input gradients and weight gradients of the layer must be BIT-identical for every order 0..5, also where the
    launch takes every XCD (groups = 8: B = 64 bidirectional / B = 128, where the shipped rule keeps order 0 and the development switch
    "xcd_interleave_force" applies the order all the same), at both precisions, with the weight-gradient side stream on (its xcd_allow masks
    follow the order) and three repetitions per order (a placement-dependent race would show as a difference between repetitions too)."""
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    G = {"lstm": 4, "gru": 3}[kind]
    torch.manual_seed(5)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    old_order, old_force = ops.get_option("xcd_interleave"), ops.get_option("xcd_interleave_force")
    runs = {}
    try:
        ops.set_option("xcd_interleave_force", 1)
        for order in (0, 1, 2, 3, 4, 5):
            ops.set_option("xcd_interleave", order)
            for rep in range(3):
                xs = x.clone().requires_grad_(True)
                ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
                y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], kind)
                y.backward(dy)
                ops.join_side_stream()
                torch.cuda.synchronize()
                ops.check_health(dev)
                runs[(order, rep)] = [y.detach().clone(), xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None]
                kernels = ops.rnn_last_kernels()
                assert "step" not in kernels[0] + kernels[1], kernels            # the persistent kernels: the per-timestep ones have no placement
    finally:
        ops.set_option("xcd_interleave", old_order)
        ops.set_option("xcd_interleave_force", old_force)
    base = runs[(0, 0)]
    assert all(torch.isfinite(t).all() for t in base)
    for key, got in runs.items():
        for i, (a, b) in enumerate(zip(got, base)):
            assert torch.equal(a, b), "order %d repetition %d: tensor %d differs from order 0 (max |d| %.3e)" % (key[0], key[1], i, float((a - b).abs().max()))


@pytest.mark.parametrize("kind,T,B,I,H,bi,sleeps", [("gru", 40, 64, 24, 512, True, 48), ("lstm", 50, 32, 40, 320, True, 48), ("lstm", 30, 64, 16, 512, True, 24),
                                                    ("gru", 25, 9, 16, 128, True, 96), ("lstm", 33, 40, 16, 384, False, 48)])
def test_rnn_fwd_tagged_with_slow_item_waves(dev, kind, T, B, I, H, bi, sleeps):
    """Round 6, the cfg4 trajectory divergence: rnn_fwd_tagged has ONE barrier per step, so its exchange waves enter step
    s + 1 while the item waves still read the parked partial tiles of step s.  With a single set of tiles only time kept a fast exchange wave
    from parking step s + 1 over them, and at a direction's first step (code not yet in the instruction cache) the item waves could lose that
    race: their pre-activations of step 0 picked up partial products of step 1.  The tiles are double buffered by step parity now; option
    "rnn_slow_items" runs the kernel's SLOW instantiation, whose item waves sleep N x 64 cycles before they read the tiles at EVERY step -- far
    beyond the ~1 000 cycles an exchange wave needs to get there.  Outputs, saved state (through the gradients) and gradients must be
    bit-identical to the undelayed run.  (tools/libctcn_single.so -- the same source with -DCTCN_RED_SINGLE, the single set of rounds 2-5 -- fails
    this test on cfg4's and cfg2's shapes on every box, on two more on some: profiles/r06_divergence_root_cause.txt.)"""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    G = {"lstm": 4, "gru": 3}[kind]
    torch.manual_seed(13)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    runs = []
    try:
        for slow, slow_x in ((0, 0), (sleeps, 0), (0, sleeps), (sleeps // 2, sleeps)):
            ops.set_option("rnn_slow_items", slow)
            ops.set_option("rnn_slow_exchange", slow_x)
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], kind)
            y.backward(dy)
            ops.join_side_stream()
            torch.cuda.synchronize()
            ops.check_health(dev)
            assert ops.rnn_last_kernels()[0] == "rnn_fwd_tagged", ops.rnn_last_kernels()
            runs.append([y.detach().clone(), xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None])
    finally:
        ops.set_option("rnn_slow_items", 0)
        ops.set_option("rnn_slow_exchange", 0)
    assert all(torch.isfinite(t).all() for t in runs[0])
    for k, got in enumerate(runs[1:]):
        for i, (a, b) in enumerate(zip(got, runs[0])):
            assert torch.equal(a, b), "run %d (%s waves delayed): tensor %d differs from the undelayed run (max |d| %.3e)" % (
                k + 1, ("item", "exchange", "item and exchange")[k], i, float((a - b).abs().max()))


@pytest.mark.parametrize("kind,T,B,I,H,bi,gather,drop", [("lstm", 50, 32, 40, 320, True, 1, 0.0), ("gru", 40, 64, 24, 512, True, 1, 0.0), ("lstm", 30, 64, 16, 512, True, 1, 0.2),
                                                         ("lstm", 50, 32, 40, 320, True, 2, 0.1), ("gru", 25, 9, 16, 128, True, 0, 0.0), ("lstm", 33, 40, 16, 384, False, 1, 0.0)])
def test_rnn_bwd_with_slow_waves(dev, kind, T, B, I, H, bi, gather, drop):
    """The backward recurrences under the same harness as test_rnn_fwd_tagged_with_slow_item_waves: rnn_bwd_scatter (two barriers per step: parked tiles,
    staged operand) and rnn_bwd_scatter2 (one barrier; operand, float32 copy and reserve rings double / triple buffered) in their SLOW instantiations --
    item waves sleep before they read the parked tiles / start their gather, exchange waves behind the barrier before they read the staged operand,
    at every step; separately and together.  Input and weight gradients must be bit-identical to the undelayed run (`gather`: option bwd_item_gather --
    0 rnn_bwd_scatter always, 1 the shipped rule, 2 rnn_bwd_scatter2 always)."""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    G = {"lstm": 4, "gru": 3}[kind]
    torch.manual_seed(17)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.2, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    runs, kernels = [], []
    try:
        ops.set_option("bwd_item_gather", gather)
        for slow, slow_x in ((0, 0), (48, 0), (0, 48), (24, 64)):
            ops._drop_counter[0] = 0
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], kind, True, drop)
            torch.cuda.synchronize()
            ops.set_option("rnn_slow_items", slow)                 # (the delays apply to the backward pass only: the forward pass has its own test)
            ops.set_option("rnn_slow_exchange", slow_x)
            y.backward(dy)
            ops.join_side_stream()
            torch.cuda.synchronize()
            ops.set_option("rnn_slow_items", 0)
            ops.set_option("rnn_slow_exchange", 0)
            ops.check_health(dev)
            kernels.append(ops.rnn_last_kernels()[1])
            runs.append([xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None])
    finally:
        ops.set_option("rnn_slow_items", 0)
        ops.set_option("rnn_slow_exchange", 0)
        ops.set_option("bwd_item_gather", 1)
    assert all(k in ("rnn_bwd_scatter", "rnn_bwd_scatter2") for k in kernels), kernels
    assert all(torch.isfinite(t).all() for t in runs[0])
    for k, got in enumerate(runs[1:]):
        for i, (a, b) in enumerate(zip(got, runs[0])):
            assert torch.equal(a, b), "%s, run %d (%s waves delayed): gradient %d differs from the undelayed run (max |d| %.3e)" % (
                kernels[0], k + 1, ("item", "exchange", "item and exchange")[k], i, float((a - b).abs().max()))


@pytest.mark.parametrize("kind,T,B,I,H,bi", [("lstm", 2, 1, 4, 8, True), ("gru", 3, 17, 8, 40, True), ("rnn", 5, 3, 4, 16, False), ("lstm", 2, 64, 16, 512, True),
                                            ("gru", 7, 2, 4, 24, False)])
def test_rnn_bwd_item_gather_edge_shapes(dev, kind, T, B, I, H, bi):
    """rnn_bwd_scatter2 and the RSV forward at the edges: two or three timesteps (shorter than the 3-deep reserve ring), one row, one slice
    (H = 8: a quarter of a tile), one direction, and the largest group count -- against the per-timestep kernels."""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    G = {"lstm": 4, "gru": 3, "rnn": 1}[kind]
    torch.manual_seed(3)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(G * H, I, device=dev) * 0.3, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)]
    w += [torch.randn(G * H, I, device=dev) * 0.3, torch.randn(G * H, H, device=dev) * (1.0 / H ** 0.5)] if bi else [None, None]
    dy = torch.randn(T, B, (2 if bi else 1) * H, device=dev)
    runs = {}
    try:
        for mode in (0, 1):
            ops.set_rnn_persistent(mode)
            ops.set_option("bwd_item_gather", 2)
            ops.set_option("fwd_rsv_lds", 1)
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) if t is not None else None for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], {"rnn": "tanh"}.get(kind, kind))
            y.backward(dy)
            torch.cuda.synchronize()
            ops.check_health(dev)
            runs[mode] = (y.detach().clone(), [xs.grad.clone()] + [t.grad.clone() for t in ws if t is not None], ops.rnn_last_kernels())
    finally:
        ops.set_rnn_persistent(1)
        ops.set_option("bwd_item_gather", 1)
        ops.set_option("fwd_rsv_lds", 2)
    assert runs[1][2][1] == "rnn_bwd_scatter2", runs[1][2]
    assert maxabs(runs[1][0], runs[0][0]) < 2e-5            # (the tagged forward carries h at 2^-16 relative; the per-timestep kernel at f32)
    for g0, g1 in zip(runs[0][1], runs[1][1]):
        assert torch.isfinite(g1).all()
        assert rel_l2(g1, g0) < 1e-4, rel_l2(g1, g0)


def test_rnn_bwd_item_gather_past_4gb_reserve(dev):
    """VERDICT r2 #7 (the backward half): a gate reserve of 4.3 GB (T = 6 600, B = 64, 2 x 4 x 320) -- beyond the one 32-bit buffer resource
    the other persistent kernels address a reserve through -- runs on rnn_bwd_scatter2 (64-bit reserve addresses, LDS-DMA reserve loads)
    and agrees with the per-timestep kernels (both forward passes run per timestep: the forward kernels keep the 4-GB limit)."""
    from ctc_pytorch_amd import ops
    ops.set_precision(1)
    T, B, I, H = 6600, 64, 8, 320
    assert T * B * 2 * 4 * H * 4 >= 1 << 32
    torch.manual_seed(5)
    x = torch.randn(T, B, I, device=dev)
    w = [torch.randn(4 * H, I, device=dev) * 0.3, torch.randn(4 * H, H, device=dev) * (0.5 / H ** 0.5),
         torch.randn(4 * H, I, device=dev) * 0.3, torch.randn(4 * H, H, device=dev) * (0.5 / H ** 0.5)]
    dy = torch.randn(T, B, 2 * H, device=dev)
    runs = {}
    try:
        for persistent in (0, 1):
            ops.set_rnn_persistent(persistent)
            xs = x.clone().requires_grad_(True)
            ws = [t.clone().requires_grad_(True) for t in w]
            y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], "lstm")
            y.backward(dy)
            torch.cuda.synchronize()
            ops.check_health(dev)
            runs[persistent] = ([xs.grad.clone()] + [t.grad.clone() for t in ws], ops.rnn_last_kernels())
            del xs, ws, y
    finally:
        ops.set_rnn_persistent(1)
    assert runs[1][1] == ("rnn_fwd_step", "rnn_bwd_scatter2"), runs[1][1]
    assert runs[0][1] == ("rnn_fwd_step", "rnn_bwd_step")
    for g0, g1 in zip(runs[0][0], runs[1][0]):
        assert torch.isfinite(g1).all()
        assert rel_l2(g1, g0) < 2e-5, rel_l2(g1, g0)


def test_rnn_c_abi_rejects_unaligned_hidden(dev):
    """The C ABI states its contract (H % 4 == 0: rows move in 16-byte pieces) and says so instead of misbehaving."""
    from ctc_pytorch_amd import ops
    x = torch.zeros(3, 2, 5, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.rnn_layer(x, torch.zeros(4 * 6, 5, device=dev), torch.zeros(4 * 6, 6, device=dev), None, None, "lstm")


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("kind,H,bi", [("LSTM", 6, True), ("GRU", 10, True), ("RNN", 7, False), ("LSTM", 321, True)])
def test_rnn_module_any_hidden_size(dev, kind, H, bi, prec):
    """nn.LSTM / GRU / RNN of the reference take every hidden size (model_ctc.py:24-25); sizes that are not multiples of 4 run
    zero-padded to the next multiple: outputs and all gradients equal the torch CPU layer."""
    from ctc_pytorch_amd import nn, ops
    ops.set_precision(prec)
    T, B, I = (9, 5, 12) if H < 100 else (40, 32, 40)
    torch.manual_seed(H)
    ref = getattr(tnn, kind)(I, H, bidirectional=bi, bias=False)
    m = getattr(nn, kind)(I, H, bidirectional=bi, bias=False)
    m.load_state_dict(ref.state_dict())
    m = m.to(dev)
    x, dy = torch.randn(T, B, I), torch.randn(T, B, (2 if bi else 1) * H)
    xr = x.clone().requires_grad_(True)
    yr, _ = ref(xr)
    yr.backward(dy)
    xg = x.to(dev).requires_grad_(True)
    y, _ = m(xg)
    assert tuple(y.shape) == tuple(yr.shape) and maxabs(y, yr) < (2e-5 if prec == 0 else 1e-4)
    y.backward(dy.to(dev))
    tol = 1e-4 if prec == 0 else 5e-4
    assert rel_l2(xg.grad, xr.grad) < tol
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_l2(p.grad, q.grad) < tol, n


def test_batchnorm_golden(dev):
    from ctc_pytorch_amd import ops
    z = load("bn_tb")
    C = z["gamma"].shape[0]
    gamma, beta = gpu(z["gamma"], dev).requires_grad_(True), gpu(z["beta"], dev).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    for step in range(2):
        x = gpu(z["x%d" % step], dev).requires_grad_(True)
        T, B, _ = x.shape
        gamma.grad = beta.grad = None
        y = ops.batch_norm(x, gamma, beta, rm, rv, T * B, C, 1, True)
        assert maxabs(y, z["y%d" % step]) < 5e-6
        y.backward(gpu(z["dy%d" % step], dev))
        assert maxabs(x.grad, z["dx%d" % step]) < 5e-6
        assert maxabs(gamma.grad, z["dgamma%d" % step]) < 5e-5
        assert maxabs(beta.grad, z["dbeta%d" % step]) < 5e-5
        assert maxabs(rm, z["rm%d" % step]) < 1e-6 and maxabs(rv, z["rv%d" % step]) < 1e-6
    xe = gpu(z["x_eval"], dev)
    T, B, _ = xe.shape
    ye = ops.batch_norm(xe, gamma, beta, rm, rv, T * B, C, 1, False)
    assert maxabs(ye, z["y_eval"]) < 5e-6


def test_batchnorm_large_rows_vs_torch(dev):
    from ctc_pytorch_amd import ops
    torch.manual_seed(0)
    x = (torch.randn(800 * 32, 640) * 3 + 1.5)
    g, b = torch.rand(640) + 0.5, torch.randn(640)
    dy = torch.randn(800 * 32, 640)
    bn = tnn.BatchNorm1d(640)
    with torch.no_grad():
        bn.weight.copy_(g); bn.bias.copy_(b)
    xr = x.clone().requires_grad_(True)
    yr = bn(xr)
    yr.backward(dy)
    xg = x.to(dev).requires_grad_(True)
    gg, bg = g.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    rm, rv = torch.zeros(640, device=dev), torch.ones(640, device=dev)
    y = ops.batch_norm(xg, gg, bg, rm, rv, x.shape[0], 640, 1, True)
    y.backward(dy.to(dev))
    assert maxabs(y, yr) < 2e-5 and maxabs(xg.grad, xr.grad) < 2e-5
    assert rel_l2(gg.grad, bn.weight.grad) < 1e-5 and rel_l2(bg.grad, bn.bias.grad) < 1e-5
    assert maxabs(rm, bn.running_mean) < 1e-5 and maxabs(rv, bn.running_var) < 1e-5


# name: (outer, C, inner, variant)   variant: None | "rows4_off" (option bn_rows4 = 0, held bit for bit to = 1) | "offset" (x at storage offset 1)
BN_BRANCH_CASES = {
    "rows_c14": (1000, 14, 1, None),            # C % 4 != 0: dword column sums, bn_apply_kernel / bn_dx_kernel (V = 1) on rows
    "rows_c62": (2001, 62, 1, None),
    "rows_c321": (777, 321, 1, None),           # ragged 64-column blocks
    "rows_c640_dword": (3000, 640, 1, "rows4_off"),
    "rows_c64_offset1": (1500, 64, 1, "offset"),    # 4-B aligned base: the dword kernels although C % 4 == 0
    "nchw_ich3": (2, 8, 40000, None),           # few planes: each cut into ich = 3 inner pieces
    "nchw_opc4": (200, 64, 37, None),           # many planes: opc = 4 planes per chunk
    "nchw_vec0": (3, 16, 399, None),            # inner % 4 != 0: scalar loads
}


def _bn_gpu(dev, x0, g0, b0, dy0, rm0, rv0, outer, C, inner, relu, offset):
    from ctc_pytorch_amd import ops
    if offset:
        buf = torch.zeros(x0.size + 1, device=dev)
        buf[1:].copy_(torch.from_numpy(x0).reshape(-1))
        x = buf[1:].view(x0.shape)
        assert x.data_ptr() % 16 == 4
    else:
        x = torch.from_numpy(x0).to(dev)
    x.requires_grad_(True)
    g = torch.from_numpy(g0).to(dev).requires_grad_(True)
    b = torch.from_numpy(b0).to(dev).requires_grad_(True)
    rm, rv = torch.from_numpy(rm0).to(dev), torch.from_numpy(rv0).to(dev)
    y = ops.batch_norm(x, g, b, rm, rv, outer, C, inner, True, 0.1, 1e-5, relu)
    y.backward(torch.from_numpy(dy0).to(dev))
    ye = ops.batch_norm(x.detach(), g.detach(), b.detach(), rm, rv, outer, C, inner, False, 0.1, 1e-5, relu)
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in (y, x.grad, g.grad, b.grad, rm, rv, ye)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", sorted(BN_BRANCH_CASES))
def test_batchnorm_branch_matrix_vs_oracle(dev, case, relu):
    """BatchNorm's launch branches that the model shapes never take -- dword column sums (C % 4 != 0, a 4-B aligned base, bn_rows4 = 0),
    bn_apply_kernel / bn_dx_kernel on rows, NCHW chunking with ich > 1 / opc > 1, NCHW without 16-B loads -- against oracle/np_ref.py in
    float64: training forward (+ ReLU), dx / dgamma / dbeta, the running statistics, the eval forward from them.  Gates of
    test_batchnorm_large_rows_vs_torch: outputs and dx 2e-5 absolute (scaled by magnitude), dgamma / dbeta rel-L2 1e-5."""
    from ctc_pytorch_amd import ops
    outer, C, inner, variant = BN_BRANCH_CASES[case]
    rs = np.random.RandomState(outer + 7 * C + inner)
    shape = (outer, C) if inner == 1 else (outer, C, inner)
    x0 = (rs.standard_normal(shape) * 2.5 + rs.standard_normal((1, C) + (1,) * (len(shape) - 2))).astype(np.float32)
    g0 = (rs.random_sample(C) + 0.5).astype(np.float32)
    b0 = (rs.standard_normal(C) * 0.3).astype(np.float32)
    dy0 = rs.standard_normal(shape).astype(np.float32)
    rm0 = (rs.standard_normal(C) * 0.1).astype(np.float32)
    rv0 = (rs.random_sample(C) + 0.5).astype(np.float32)
    if variant == "rows4_off":
        ops.set_option("bn_rows4", 0)
        try:
            got = _bn_gpu(dev, x0, g0, b0, dy0, rm0, rv0, outer, C, inner, relu, False)
        finally:
            ops.set_option("bn_rows4", 1)
        # (the two kernels' float64 column sums agree to float64 rounding and reach every output through float32)
        for a, c in zip(got, _bn_gpu(dev, x0, g0, b0, dy0, rm0, rv0, outer, C, inner, relu, False)):
            assert torch.equal(a, c)
    else:
        got = _bn_gpu(dev, x0, g0, b0, dy0, rm0, rv0, outer, C, inner, relu, variant == "offset")
    y, dx, dg, db, rm, rv, ye = got
    to2 = lambda a: np.asarray(a, dtype=np.float64).reshape(outer, C, inner).transpose(0, 2, 1).reshape(-1, C)
    x2, dy2 = to2(x0), to2(dy0)
    n = x2.shape[0]
    y_ref, mean, var = R.bn_train_fwd(x2, g0.astype(np.float64), b0.astype(np.float64))
    mask = np.ones_like(y_ref)
    if relu:
        mask = (to2(y.numpy()) > 0).astype(np.float64)         # the kernel's own ReLU mask (float32 values at 0 can fall either way) ...
        sure = np.abs(y_ref) > 1e-4
        assert np.array_equal(mask[sure], (y_ref[sure] > 0).astype(np.float64))     # ... which is the oracle's away from 0
        y_ref = np.maximum(y_ref, 0.0)
    dx_ref, dg_ref, db_ref = R.bn_train_bwd(x2, g0.astype(np.float64), mean, var, dy2 * mask)
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    assert maxabs(to2(y.numpy()), y_ref) < 2e-5 * scale(y_ref)
    assert maxabs(to2(dx.numpy()), dx_ref) < 2e-5 * scale(dx_ref)
    assert rel_l2(dg, dg_ref) < 1e-5 and rel_l2(db, db_ref) < 1e-5
    rm_ref, rv_ref = R.bn_running_update(rm0.astype(np.float64), rv0.astype(np.float64), mean, var, n, 0.1)
    assert maxabs(rm, rm_ref) < 1e-5 * scale(rm_ref) and maxabs(rv, rv_ref) < 1e-5 * scale(rv_ref)
    ye_ref = R.bn_eval_fwd(x2, g0.astype(np.float64), b0.astype(np.float64), rm.numpy().astype(np.float64), rv.numpy().astype(np.float64))
    if relu:
        ye_ref = np.maximum(ye_ref, 0.0)
    assert maxabs(to2(ye.numpy()), ye_ref) < 2e-5 * scale(ye_ref)


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 128, 129, 200, 1000, 4097])
def test_log_softmax_argmax_edges_vs_oracle(dev, V):
    """ops.log_softmax forward / backward and ctcn_argmax (alone, and fused into ctcn_log_softmax_fwd) at class counts either side of the
    64-lane wave, 1 and 4 097, on 23 rows (no multiple of the 4 rows per workgroup): Gaussian rows, exact ties (logits quantised to
    integers), rows with -inf entries, rows shifted by +-1e4.  Against oracle/np_ref.py in float64, per row with eps = 2^-23:
      log-probs: 4 eps (|max z| + ln V + 1) -- the float32 rounding of max + ln(sum) and of x - lse -- plus (V / 64 + 8) eps for the
      float32 sum of exp (V / 64 terms per lane, six butterfly levels, 1-ulp expf);
      dlogits (against log_softmax_bwd of the kernel's own log-probs): 4 eps (max|g| + max p (V / 64 + 8) sum|g|) -- the float32 sum of g
      and the rounding of g - p * sum;
      -inf entries stay -inf with dlogits = g.  The arg-max equals np_ref.argmax_first of the kernel's own log-probs exactly (lowest
      index on ties)."""
    from ctc_pytorch_amd import _lib, ops
    rs = np.random.RandomState(V)
    rows = 23
    z = rs.standard_normal((rows, V)) * 3.0
    z[3:8] = np.round(z[3:8] / 2.0)                         # exact ties
    if V > 1:
        for r in range(8, 12):                              # -inf entries (the row's first maximum stays finite)
            k = rs.randint(0, V, size=max(1, V // 3))
            z[r, k] = -np.inf
            z[r, rs.randint(0, V)] = 5.0
        z[12:15] += 1e4
        z[15:18] -= 1e4
        z[18, :] = 0.0                                      # all equal: arg-max 0
    z = z.astype(np.float32)
    g = rs.standard_normal((rows, V)).astype(np.float32)
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    lp = ops.log_softmax(zt)
    lp.backward(torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    L = _lib.lib()
    am = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    assert L.ctcn_argmax(ctypes.c_void_p(lp.data_ptr()), ctypes.c_void_p(am.data_ptr()), rows, V, None) == 0
    lp2 = torch.empty_like(lp)
    am2 = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    assert L.ctcn_log_softmax_fwd(ctypes.c_void_p(zt.data_ptr()), ctypes.c_void_p(lp2.data_ptr()), ctypes.c_void_p(am2.data_ptr()), rows, V, None) == 0
    torch.cuda.synchronize()
    lp_k = lp.detach().cpu().numpy()
    dz = zt.grad.cpu().numpy().astype(np.float64)
    assert np.array_equal(lp2.cpu().numpy(), lp_k)
    eps = 2.0 ** -23
    fin = np.isfinite(z)
    with np.errstate(invalid="ignore"):
        lp_ref = R.log_softmax(z)
    assert np.array_equal(np.isfinite(lp_k), fin) and np.all(lp_k[~fin] == -np.inf)
    zmax = np.abs(np.where(fin, z, 0.0)).max(axis=1)
    tol_lp = 4 * eps * (zmax + np.log(V) + 1.0) + (V / 64 + 8) * eps
    err_lp = np.where(fin, np.abs(lp_k.astype(np.float64) - np.where(fin, lp_ref, 0.0)), 0.0).max(axis=1)
    assert np.all(err_lp <= tol_lp), (err_lp / tol_lp).max()
    dz_ref = R.log_softmax_bwd(lp_k.astype(np.float64), g.astype(np.float64))
    p = np.exp(lp_k.astype(np.float64))
    g64 = np.abs(g.astype(np.float64))
    tol_dz = 4 * eps * (g64.max(axis=1) + p.max(axis=1) * (V / 64 + 8) * g64.sum(axis=1))
    assert np.all(np.abs(dz - dz_ref).max(axis=1) <= tol_dz)
    assert np.array_equal(dz[~fin], g.astype(np.float64)[~fin])
    want = R.argmax_first(lp_k)
    assert np.array_equal(am.cpu().numpy(), want) and np.array_equal(am2.cpu().numpy(), want)
    if V > 1:
        assert np.array_equal(want[18:19], [0])


def _load_conv_model(dev):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    z = load("conv_front_relu")
    cnn_param = {"batch_norm": True, "activate_function": nn.ReLU,
                 "layer": [[(1, 32), (3, 3), (1, 2), (1, 1), None], [(32, 32), (3, 3), (2, 2), (1, 1), None]]}
    rnn_param = {"rnn_input_size": 40, "rnn_hidden_size": 16, "rnn_layers": 1, "rnn_type": nn.LSTM, "bidirectional": True,
                 "batch_norm": True}
    m = CTC_Model(add_cnn=True, cnn_param=cnn_param, rnn_param=rnn_param, num_class=12, drop_out=0.0)
    sd = m.state_dict()
    for k in list(sd.keys()):
        if k.startswith("conv."):
            kk = k[len("conv."):]
            src = z["w." + kk] if ("w." + kk) in z.files else None
            if src is not None:
                sd[k] = torch.from_numpy(src)
            # running stats of the fixture are post-step values; start from the defaults instead
    m.load_state_dict(sd)
    return m.to(dev), z


@pytest.mark.parametrize("rows,C,inner,relu", [(3000, 640, 1, False), (24, 32, 21 * 20, True)])
def test_sync_batchnorm_two_shards_equal_full_batch(dev, rows, C, inner, relu):
    """BatchNorm statistics over the GLOBAL batch.  Two 'ranks' hold halves of a batch; their per-channel
    fp64 sums are added (what the all-reduce does) and each finishes with the global count: outputs, running stats and
    dx equal the single-process BatchNorm of the whole batch, dgamma / dbeta add up to it."""
    from ctc_pytorch_amd import _lib, ops
    L = _lib.lib()
    rs = np.random.RandomState(rows + C)
    shape = (rows, C) if inner == 1 else (rows, C, inner)
    x = torch.from_numpy((rs.standard_normal(shape) * 1.7 + 0.3).astype(np.float32)).to(dev)
    dy = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dev)
    g = torch.from_numpy((1 + 0.1 * rs.standard_normal(C)).astype(np.float32)).to(dev)
    b = torch.from_numpy((0.1 * rs.standard_normal(C)).astype(np.float32)).to(dev)
    # single process
    xg, gg, bg = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = ops.batch_norm(xg, gg, bg, rm, rv, rows, C, inner, True, relu=relu)
    y.backward(dy)
    # two shards through the sync path, with a reducer that adds the other shard's sums
    h = rows // 2
    parts = [(x[:h].contiguous(), dy[:h].contiguous()), (x[h:].contiguous(), dy[h:].contiguous())]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = _lib.workspace(dev)
    wp, wn = ctypes.c_void_p(ws.data_ptr()), ws.numel()
    st = _lib.stream_ptr()
    sums = [torch.empty((C, 2), dtype=torch.float64, device=dev) for _ in parts]
    for (xs, _), sm in zip(parts, sums):
        _lib.check(L.ctcn_bn_fwd_sums(ptr(xs), ptr(sm), xs.shape[0], C, inner, wp, wn, st), "sums")
    glob = sums[0] + sums[1]
    total = float(rows * inner)
    ys, means, rstds, rms, rvs = [], [], [], [], []
    for xs, _ in parts:
        yy, mean, rstd = torch.empty_like(xs), torch.empty(C, device=dev), torch.empty(C, device=dev)
        rm2, rv2 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        _lib.check(L.ctcn_bn_fwd_finish(ptr(xs), ptr(yy), ptr(g), ptr(b), ptr(rm2), ptr(rv2), ptr(mean), ptr(rstd), ptr(glob), total,
                                        xs.shape[0], C, inner, 1e-5, 0.1, int(relu), st, None), "finish")
        ys.append(yy); means.append(mean); rstds.append(rstd); rms.append(rm2); rvs.append(rv2)
    assert maxabs(torch.cat(ys), y) < 2e-6
    assert maxabs(rms[0], rm) < 1e-7 and maxabs(rvs[1], rv) < 1e-6 and maxabs(rms[0], rms[1]) == 0
    lsum = [torch.empty((C, 2), dtype=torch.float64, device=dev) for _ in parts]
    for (xs, ds), yy, mean, rstd, sm in zip(parts, ys, means, rstds, lsum):
        _lib.check(L.ctcn_bn_bwd_sums(ptr(xs), ptr(yy), ptr(ds), ptr(mean), ptr(rstd), ptr(sm), xs.shape[0], C, inner, int(relu), wp, wn, st), "bsums")
    gsum = lsum[0] + lsum[1]
    dxs, dgs, dbs = [], [], []
    for (xs, ds), yy, mean, rstd, sm in zip(parts, ys, means, rstds, lsum):
        dx, dg, db = torch.empty_like(xs), torch.empty(C, device=dev), torch.empty(C, device=dev)
        _lib.check(L.ctcn_bn_bwd_finish(ptr(xs), ptr(yy), ptr(ds), ptr(g), ptr(mean), ptr(rstd), ptr(dx), ptr(dg), ptr(db), ptr(sm), ptr(gsum),
                                        total, xs.shape[0], C, inner, int(relu), 0.0, wp, wn, st), "bfinish")
        dxs.append(dx); dgs.append(dg); dbs.append(db)
    assert maxabs(torch.cat(dxs), xg.grad) < 2e-6
    assert rel_l2(dgs[0] + dgs[1], gg.grad) < 1e-6 and rel_l2(dbs[0] + dbs[1], bg.grad) < 1e-6
    # the autograd path with a 1-rank reducer is the plain BatchNorm
    ops.set_sync_bn(lambda sm, n: float(n))
    try:
        x2, g2, b2 = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y2 = ops.batch_norm(x2, g2, b2, torch.zeros(C, device=dev), torch.ones(C, device=dev), rows, C, inner, True, relu=relu)
        y2.backward(dy)
    finally:
        ops.set_sync_bn(None)
    assert maxabs(y2, y) < 1e-6 and maxabs(x2.grad, xg.grad) < 1e-6 and rel_l2(g2.grad, gg.grad) < 1e-6


CONV_CASES = [  # B, Ci, Hi, Wi, Co, kh, kw, sh, sw, ph, pw
    (3, 1, 37, 40, 32, 3, 3, 1, 2, 1, 1),      # the reference's first layer shape (ctc_config.yaml)
    (2, 32, 21, 20, 32, 3, 3, 2, 2, 1, 1),     # its second layer
    (2, 3, 9, 11, 5, 3, 2, 1, 1, 0, 1),        # K = 18, Co = 5: ragged in both MFMA dimensions
    (1, 7, 5, 6, 17, 1, 1, 1, 1, 0, 0),        # 1x1 taps, Co just over one 16-column tile
    (2, 2, 4, 4, 64, 5, 5, 2, 3, 2, 2),        # taps wider than the image, widest filter bank
    (1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0),         # a single output position
    (5, 16, 13, 7, 48, 3, 3, 1, 1, 1, 1),
    # (round 6) filter banks no kernel holds in LDS as a whole: the direct kernels run them as (output channels, input channels) slices
    (2, 1, 9, 60, 32, 3, 41, 1, 2, 0, 0),      # the reference's example front-end (model_ctc.py:232-233), layer 1: 123 taps
    (2, 32, 12, 30, 32, 3, 21, 2, 2, 0, 0),    # ... layer 2: 32 x 32 x 3 x 21 = 258 KB of filters
    (1, 20, 6, 9, 70, 5, 5, 1, 2, 2, 1),       # more than 64 output channels, 140 KB, ragged slices
    (1, 3, 40, 40, 2, 29, 29, 3, 2, 14, 14),   # 841 taps per channel pair (the direct kernels' limit is ~900): one-channel slices in the weight gradient
    # more than 256 output channels: the direct weight-gradient kernel's 256 threads hold one bias column each (launches of <= 256 channels)
    (2, 1, 9, 40, 300, 1, 11, 1, 1, 0, 5),     # a Conv1d-like front end, bank unsliced
    (1, 1, 5, 64, 512, 1, 11, 1, 2, 0, 5),
    (2, 3, 7, 9, 260, 3, 3, 1, 1, 1, 1),
    (1, 4, 6, 20, 300, 3, 3, 1, 1, 1, 1),      # 10 800 taps > 256 * WPT: the sliced weight gradient (284 channels per slice before the clamp)
]
_CONV_WIDE = CONV_CASES[-4:]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("mfma", [1, 0])
def test_conv2d_vs_oracle(dev, case, mfma):
    """ctcn_conv2d_fwd / _bwd (torch.nn.Conv2d of model/cnn.py:32-38 in the reference) against the float64 oracle
    (oracle/np_ref.py conv2d_fwd / conv2d_bwd): the MFMA implicit-GEMM kernels (default) and the direct kernels
    (option conv_mfma = 0) under the same float32 gate, on ragged shapes either side of the 16 / 4 / 64 tile edges."""
    from ctc_pytorch_amd import _lib, ops
    B, Ci, Hi, Wi, Co, kh, kw, sh, sw, ph, pw = case
    rs = np.random.RandomState(sum(case))
    x = rs.standard_normal((B, Ci, Hi, Wi)).astype(np.float32)
    w = (rs.standard_normal((Co, Ci, kh, kw)) / np.sqrt(Ci * kh * kw)).astype(np.float32)
    b = rs.standard_normal(Co).astype(np.float32)
    y_ref = R.conv2d_fwd(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), (sh, sw), (ph, pw))
    dy = rs.standard_normal(y_ref.shape).astype(np.float32)
    dx_ref, dw_ref, db_ref = R.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), (sh, sw), (ph, pw), dy.astype(np.float64))
    _lib.lib().ctcn_set_option(b"conv_mfma", mfma)
    try:
        xt = torch.from_numpy(x).to(dev).requires_grad_()
        wt = torch.from_numpy(w).to(dev).requires_grad_()
        bt = torch.from_numpy(b).to(dev).requires_grad_()
        y = ops.conv2d(xt, wt, bt, (sh, sw), (ph, pw))
        y.backward(torch.from_numpy(dy).to(dev))
        torch.cuda.synchronize()
    finally:
        _lib.lib().ctcn_set_option(b"conv_mfma", 1)
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    assert tuple(y.shape) == y_ref.shape
    assert maxabs(y, y_ref) < 2e-6 * scale(y_ref) * np.sqrt(Ci * kh * kw)
    assert maxabs(xt.grad, dx_ref) < 2e-6 * scale(dx_ref) * np.sqrt(Co * kh * kw)
    assert rel_l2(wt.grad, dw_ref) < 2e-6 and rel_l2(bt.grad, db_ref) < 2e-6


@pytest.mark.parametrize("case", _CONV_WIDE)
@pytest.mark.parametrize("mfma", [1, 0])
def test_conv2d_bwd_wide_bias_from_nan_workspace(dev, case, mfma):
    """ctcn_conv2d_bwd called directly with its workspace, dw and dbias filled with NaN beforehand: every partial the reduction reads must
    have been written by this call (a bias column left unwritten -- output channels >= 256 -- shows as NaN whatever the caching allocator
    would have left there).  dx, dw and dbias against the float64 oracle under test_conv2d_vs_oracle's gates."""
    from ctc_pytorch_amd import _lib
    B, Ci, Hi, Wi, Co, kh, kw, sh, sw, ph, pw = case
    rs = np.random.RandomState(sum(case) + 1)
    x = rs.standard_normal((B, Ci, Hi, Wi)).astype(np.float32)
    w = (rs.standard_normal((Co, Ci, kh, kw)) / np.sqrt(Ci * kh * kw)).astype(np.float32)
    Ho, Wo = (Hi + 2 * ph - kh) // sh + 1, (Wi + 2 * pw - kw) // sw + 1
    dy = rs.standard_normal((B, Co, Ho, Wo)).astype(np.float32)
    dx_ref, dw_ref, db_ref = R.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), (sh, sw), (ph, pw), dy.astype(np.float64))
    L = _lib.lib()
    L.ctcn_set_option(b"conv_mfma", mfma)
    try:
        nbytes = L.ctcn_conv2d_ws_bytes(*case)
        ws = torch.full(((max(nbytes, 4) + 3) // 4,), float("nan"), dtype=torch.float32, device=dev)
        xt, wt, dyt = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
        dx = torch.full(x.shape, float("nan"), dtype=torch.float32, device=dev)
        dw = torch.full(w.shape, float("nan"), dtype=torch.float32, device=dev)
        db = torch.full((Co,), float("nan"), dtype=torch.float32, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = L.ctcn_conv2d_bwd(P(xt), P(wt), P(dyt), P(dx), P(dw), P(db), *case, 0.0, P(ws), ws.numel() * 4,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        L.ctcn_set_option(b"conv_mfma", 1)
    assert rc == 0, L.ctcn_last_error()
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    for t in (dx, dw, db):
        assert bool(torch.isfinite(t).all())
    assert maxabs(dx, dx_ref) < 2e-6 * scale(dx_ref) * np.sqrt(Co * kh * kw)
    assert rel_l2(dw, dw_ref) < 2e-6 and rel_l2(db, db_ref) < 2e-6


def test_conv1d_300_channels_vs_torch_cpu(dev):
    """nn.Conv1d(1, 300, 11) (LayerCNN's one-element kernel branch with a wide bank) forward and backward against torch's CPU Conv1d in
    float64 with the same parameters: y, dx, dweight and dbias -- the bias gradient of channels 256 .. 299 included."""
    from ctc_pytorch_amd import nn
    torch.manual_seed(11)
    ref = tnn.Conv1d(1, 300, 11).double()
    m = nn.Conv1d(1, 300, 11)
    with torch.no_grad():
        m.weight.copy_(ref.weight.float()); m.bias.copy_(ref.bias.float())
        ref.weight.copy_(m.weight.double()); ref.bias.copy_(m.bias.double())
    m = m.to(dev)
    x = torch.randn(3, 1, 57)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    dy = torch.randn(yr.shape)
    yr.backward(dy.double())
    xg = x.to(dev).requires_grad_(True)
    y = m(xg)
    y.backward(dy.to(dev))
    assert tuple(y.shape) == tuple(yr.shape)
    assert maxabs(y, yr) < 2e-6 * max(1.0, float(yr.abs().max())) * np.sqrt(11)
    assert maxabs(xg.grad, xr.grad) < 2e-6 * max(1.0, float(xr.grad.abs().max())) * np.sqrt(300 * 11)
    assert rel_l2(m.weight.grad, ref.weight.grad) < 2e-6 and rel_l2(m.bias.grad, ref.bias.grad) < 2e-6


@pytest.mark.parametrize("shape,k", [((2, 3, 9, 8), (2, 2)), ((1, 2, 7, 5), (3, 1)), ((2, 1, 4, 6), (1, 3)), ((1, 1, 5, 5), (5, 5)),
                                     ((3, 8, 121, 20), (2, 1)), ((1, 4, 16, 16), (16, 16))])
def test_maxpool2d_vs_oracle(dev, shape, k):
    """ctcn_maxpool2d_fwd / _bwd (nn.MaxPool2d(pooling_size) of LayerCNN, model_ctc.py:52-53) against oracle/np_ref.py (itself
    pinned to torch's CPU op in tests/test_oracle_golden.py), bit-exact: values, the gradient routing on ties (first maximum: the
    post-ReLU zeros of the reference path tie all the time), NaN inputs, rows / columns cut off by the floor."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(sum(shape) + k[0])
    x = np.maximum(rs.standard_normal(shape), 0).astype(np.float32)          # ReLU output: many exact ties at 0
    x.reshape(-1)[rs.randint(0, x.size, size=max(1, x.size // 40))] = np.nan
    y_ref, arg = R.maxpool2d_fwd(x, *k)
    dy = rs.standard_normal(y_ref.shape).astype(np.float32)
    dx_ref = R.maxpool2d_bwd(dy, arg, shape, *k)
    xt = torch.from_numpy(x).to(dev).requires_grad_()
    y = ops.max_pool2d(xt, k)
    y.backward(torch.from_numpy(dy).to(dev))
    assert np.array_equal(y.detach().cpu().numpy(), y_ref, equal_nan=True)
    assert np.array_equal(xt.grad.cpu().numpy(), dx_ref)
    with pytest.raises(RuntimeError):
        ops.max_pool2d(xt, (shape[2] + 1, 1))                                  # window larger than the image


@pytest.mark.parametrize("prec", [0, 1])
def test_conv_front_golden(dev, prec):
    """(the direct convolution and BatchNorm are f32 in both modes: the same f32-strict gates hold at precision 1)"""
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    m, z = _load_conv_model(dev)
    m.train()
    x = gpu(z["x"], dev).requires_grad_(True)
    c = m.conv(x.unsqueeze(1))
    assert maxabs(c, z["conv_out"]) < 2e-5
    r = ops.bctf_to_tbcf(c)
    assert tuple(r.shape) == z["rnn_in"].shape and maxabs(r, z["rnn_in"]) < 2e-5
    r.backward(gpu(z["d_rnn_in"], dev))
    assert maxabs(x.grad, z["dx"]) < 5e-5
    for k, p in m.conv.named_parameters():
        assert maxabs(p.grad, z["g." + k]) < 5e-4 * max(1.0, float(np.abs(z["g." + k]).max())), k   # (conv.bias: ~0 on both sides)
    for k, bfr in m.conv.named_buffers():
        if "num_batches" in k:
            assert int(bfr) == int(z["b." + k])
        else:
            assert maxabs(bfr, z["b." + k]) < 1e-5, k
    m.eval()
    with torch.no_grad():
        ce = m.conv(x.detach().unsqueeze(1))
    assert maxabs(ce, z["conv_out_eval"]) < 2e-5


@pytest.mark.parametrize("tag", ["a", "b"])
def test_layer_cnn_one_element_kernel_branch_golden(dev, tag):
    """LayerCNN with a one-element kernel_size (reference model_ctc.py:48-50, 54-55: Conv1d -> BatchNorm1d -> ReLU -> MaxPool1d -> Dropout)
    against tests/golden/layer_cnn1d.npz, which oracle/gen_golden.py captured from the reference's own LayerCNN: two training steps (outputs,
    input / parameter gradients, running statistics after both) and an eval pass.  "a": 5 -> 12 channels, 7 taps, stride 2, padding 3,
    pool 3, BatchNorm; "b": 3 -> 70 channels, 41 taps, pool 2, no BatchNorm (the separate ReLU module)."""
    from ctc_pytorch_amd.models.model_ctc import LayerCNN
    z = load("layer_cnn1d")
    cin, cout, k, s, p, pool, bn, L = (int(v) for v in z[tag + ".cfg"])
    layer = LayerCNN(cin, cout, (k,), (s,), (p,), pooling_size=pool, batch_norm=bool(bn), dropout=0.0)
    before = {key[len(tag + ".before."):]: z[key] for key in z.files if key.startswith(tag + ".before.")}
    assert list(layer.state_dict().keys()) == list(before.keys())
    layer.load_state_dict({key: torch.from_numpy(v) for key, v in before.items()})
    layer.to(dev).train()
    for step in range(2):
        x = gpu(z["%s.x%d" % (tag, step)], dev).requires_grad_(True)
        layer.zero_grad()
        y = layer(x)
        want = z["%s.y%d" % (tag, step)]
        assert tuple(y.shape) == want.shape and maxabs(y, want) < 2e-5
        y.backward(gpu(z["%s.dy%d" % (tag, step)], dev))
        assert maxabs(x.grad, z["%s.dx%d" % (tag, step)]) < 5e-5
        for key, q in layer.named_parameters():
            g = z["%s.g%d.%s" % (tag, step, key)]
            assert tuple(q.grad.shape) == g.shape and maxabs(q.grad, g) < 5e-4 * max(1.0, float(np.abs(g).max())), key
    for key, v in layer.state_dict().items():
        w = z["%s.after.%s" % (tag, key)]
        assert (int(v) == int(w)) if "num_batches" in key else (maxabs(v, w) < 1e-5), key
    layer.eval()
    with torch.no_grad():
        ye = layer(x.detach())
    assert maxabs(ye, z[tag + ".y_eval"]) < 2e-5
    with pytest.raises((ValueError, RuntimeError)):          # what CTC_Model.forward would feed: nn.Conv1d refuses 4-D input in the reference as well
        layer(x.detach().unsqueeze(1))


@pytest.mark.parametrize("prec", [0, 1])
def test_fc_logsoftmax_golden(dev, prec):
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    tol_act, tol_grad, _ = gates(prec, 1e-5, 1e-4, 0)
    z = load("fc_lsm")
    x = gpu(z["x"], dev).requires_grad_(True)
    g, b = gpu(z["w.0.weight"], dev).requires_grad_(True), gpu(z["w.0.bias"], dev).requires_grad_(True)
    W = gpu(z["w.1.weight"], dev).requires_grad_(True)
    C = x.shape[1]
    T, B, V = z["lp"].shape
    y = ops.batch_norm(x, g, b, torch.zeros(C, device=dev), torch.ones(C, device=dev), x.shape[0], C, 1, True)
    logits = ops.linear(y, W)
    assert maxabs(logits, z["logits"]) < tol_act
    lp = ops.log_softmax(logits.view(T, B, V))
    assert maxabs(lp, z["lp"]) < tol_act
    argmax_report(lp, z["argmax"], "fc_lsm")
    lp.backward(gpu(z["dlp"], dev))
    if prec == 0:
        assert maxabs(x.grad, z["dx"]) < 2e-5
        assert maxabs(W.grad, z["g.1.weight"]) < 1e-4 and maxabs(g.grad, z["g.0.weight"]) < 1e-4
    else:
        assert rel_l2(x.grad, z["dx"]) < tol_grad and rel_l2(W.grad, z["g.1.weight"]) < tol_grad and rel_l2(g.grad, z["g.0.weight"]) < tol_grad


def test_ctc_golden(dev):
    from ctc_pytorch_amd import nn, ops
    z = load("ctc_loss")
    B = z["lp"].shape[1]
    logits = gpu(z["logits"], dev).requires_grad_(True)
    lp = ops.log_softmax(logits)
    lp.retain_grad()
    tg, il, tl = gpu(z["targets"], dev), gpu(z["in_len"], dev), gpu(z["tgt_len"], dev)
    loss = nn.CTCLoss(reduction="sum")(lp, tg, il, tl) / B
    assert abs(float(loss.detach()) - float(z["loss"])) / float(z["loss"]) < 1e-5
    loss.backward()
    assert maxabs(lp.grad, z["dlp"]) < 1e-5
    assert maxabs(logits.grad, z["dlogits"]) < 1e-5
    nll = nn.CTCLoss(reduction="none")(lp.detach(), tg, il, tl)
    assert np.allclose(nll.cpu().numpy(), z["nll"], rtol=1e-5, atol=1e-4)
    # infeasible utterance: +inf loss, NaN gradient rows where torch has them, finite elsewhere
    lp2 = gpu(z["lp"], dev).requires_grad_(True)
    il2 = gpu(z["in_len_inf"], dev)
    l2 = nn.CTCLoss(reduction="sum")(lp2, tg, il2, tl) / B
    assert np.isinf(float(l2))
    l2.backward()
    got = lp2.grad.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(z["dlp_inf"]))
    ok = ~np.isnan(got)
    assert np.max(np.abs(got[ok] - z["dlp_inf"][ok])) < 1e-5


def test_ctc_vs_torch_cpu_random(dev):
    from ctc_pytorch_amd import nn, ops
    T, B, V = 200, 16, 62
    b = synth.make_batch(seed=9, B=B, T=T, F=4, V=V, lab_lo=10, lab_hi=60)
    rs = np.random.RandomState(3)
    logits = torch.from_numpy((2 * rs.standard_normal((T, B, V))).astype(np.float32))
    tg, tl, il = torch.from_numpy(b["targets"]), torch.from_numpy(b["tgt_len"]), torch.from_numpy(b["lens"])
    lr = logits.clone().requires_grad_(True)
    loss_r = tnn.CTCLoss(reduction="sum")(torch.log_softmax(lr, -1), tg, il, tl) / B
    loss_r.backward()
    lg = logits.to(dev).requires_grad_(True)
    loss = nn.CTCLoss(reduction="sum")(ops.log_softmax(lg), tg.to(dev), il.to(dev), tl.to(dev)) / B
    loss.backward()
    assert abs(float(loss) - float(loss_r)) / abs(float(loss_r)) < 1e-5
    assert maxabs(lg.grad, lr.grad) < 2e-5
    assert float(lg.grad.sum(-1).abs().max()) < 1e-4          # rows sum to zero after log_softmax backward


@pytest.mark.parametrize("T,B,V,lab", [(200, 16, 62, (10, 60)), (64, 5, 20, (1, 30)), (300, 3, 40, (100, 140))])
def test_ctc_one_launch_lattices_equal_two_pass_reserve(dev, T, B, V, lab):
    """ctcn_ctc_fwd_both + ctcn_ctc_grad (alpha and beta side by side in one launch: the training path) against
    ctcn_ctc_fwd + ctcn_ctc_bwd (beta accumulated into the alpha reserve): same nll and gradient, bit for bit; ragged lengths,
    one infeasible utterance (label longer than the input) included."""
    from ctc_pytorch_amd import _lib, ops
    b = synth.make_batch(seed=21, B=B, T=T, F=4, V=V, lab_lo=lab[0], lab_hi=lab[1])
    rs = np.random.RandomState(4)
    lp = ops.log_softmax(torch.from_numpy((2 * rs.standard_normal((T, B, V))).astype(np.float32)).to(dev)).contiguous()
    tg = torch.from_numpy(b["targets"]).to(dev)
    tl = torch.from_numpy(b["tgt_len"]).to(dev)
    lens = b["lens"].copy()
    lens[-1] = min(int(lens[-1]), max(1, int(b["tgt_len"][-1]) - 1))     # no alignment exists: nll = +inf
    il = torch.from_numpy(lens).to(dev)
    Lmax = tg.shape[1]
    L, P, st = _lib.lib(), (lambda t: ctypes.c_void_p(t.data_ptr())), _lib.stream_ptr()
    gs = torch.full((1,), 1.0 / B, device=dev)
    a1 = torch.empty((T, B, 2 * Lmax + 1), device=dev)
    n1, g1 = torch.empty(B, device=dev), torch.empty_like(lp)
    _lib.check(L.ctcn_ctc_fwd(P(lp), P(tg), P(il), P(tl), P(a1), P(n1), T, B, V, Lmax, st), "ctc_fwd")
    alpha_only = a1.clone()
    _lib.check(L.ctcn_ctc_bwd(P(lp), P(tg), P(il), P(tl), P(a1), P(n1), P(gs), P(g1), T, B, V, Lmax, st), "ctc_bwd")
    a2, b2 = torch.empty_like(a1), torch.empty_like(a1)
    n2, g2 = torch.empty(B, device=dev), torch.empty_like(lp)
    _lib.check(L.ctcn_ctc_fwd_both(P(lp), P(tg), P(il), P(tl), P(a2), P(b2), P(n2), T, B, V, Lmax, st), "ctc_fwd_both")
    _lib.check(L.ctcn_ctc_grad(P(lp), P(tg), P(il), P(tl), P(a2), P(b2), P(n2), P(gs), P(g2), T, B, V, Lmax, st), "ctc_grad")
    torch.cuda.synchronize()
    assert bool(torch.isinf(n1[-1])) == (int(b["tgt_len"][-1]) >= 2) and torch.equal(n1, n2)
    fin = torch.isfinite(n1).cpu().numpy()
    for i in range(B):                                  # lattice rows the passes define: t < len, s < 2*L+1
        S, Tb = 2 * int(b["tgt_len"][i]) + 1, int(lens[i])
        assert torch.equal(alpha_only[:Tb, i, :S], a2[:Tb, i, :S])
        assert torch.equal(a1[:Tb, i, :S], a2[:Tb, i, :S] + b2[:Tb, i, :S])
    assert torch.equal(g1[:, fin], g2[:, fin])
    assert torch.equal(torch.isnan(g1), torch.isnan(g2))


@pytest.mark.parametrize("T,B,V,Lmax", [(700, 5, 50, 200), (1200, 3, 30, 520), (9, 7, 12, 3), (3400, 3, 20, 1500)])
def test_ctc_long_labels_vs_torch_cpu(dev, T, B, V, Lmax):
    """Label lengths that need 2, 4+ and (L = 1500: S = 3001) 16 lattice states per thread, ragged input lengths incl.
    a 1-frame utterance, repeated labels, and an empty target."""
    from ctc_pytorch_amd import nn, ops
    rs = np.random.RandomState(T + Lmax)
    tl = rs.randint(max(1, Lmax // 2), Lmax + 1, size=B).astype(np.int64)
    tl[0] = Lmax
    tl[-1] = 0
    tg = rs.randint(1, V, size=(B, Lmax)).astype(np.int64)
    tg[1, : Lmax // 2] = tg[1, 0]                                  # long run of repeats
    il = np.minimum(T, 2 * tl + rs.randint(1, 40, size=B) + Lmax // 2).astype(np.int64)
    il[0] = T
    il[-1] = 1
    logits = torch.from_numpy((1.5 * rs.standard_normal((T, B, V))).astype(np.float32))
    lr = logits.clone().requires_grad_(True)
    loss_r = tnn.CTCLoss(reduction="sum", zero_infinity=False)(torch.log_softmax(lr, -1), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl))
    loss_r.backward()
    lg = logits.to(dev).requires_grad_(True)
    loss = nn.CTCLoss(reduction="sum")(ops.log_softmax(lg), torch.from_numpy(tg).to(dev), torch.from_numpy(il).to(dev), torch.from_numpy(tl).to(dev))
    loss.backward()
    assert np.isfinite(float(loss_r))
    assert abs(float(loss) - float(loss_r)) / abs(float(loss_r)) < 1e-5
    # alpha / beta reach |3000| here, where one f32 ulp is 2.4e-4: judge both f32 implementations against float64
    l64 = logits.double().requires_grad_(True)
    tnn.CTCLoss(reduction="sum")(torch.log_softmax(l64, -1), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)).backward()
    err_ours, err_torch32 = maxabs(lg.grad.double().cpu(), l64.grad), maxabs(lr.grad.double(), l64.grad)
    assert err_ours < max(5e-5, 3.0 * err_torch32), (err_ours, err_torch32)


def test_dropout_statistics_and_mask_reuse(dev):
    from ctc_pytorch_amd import ops
    x = torch.ones(1 << 20, device=dev, requires_grad=True)
    y = ops.dropout(x, 0.25, True)
    keep = (y != 0).float().mean().item()
    assert abs(keep - 0.75) < 5e-3
    assert torch.allclose(y[y != 0], torch.tensor(1 / 0.75, device=dev))
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad != 0, y != 0)                   # backward regenerates the same mask
    y2 = ops.dropout(x, 0.25, True)
    assert not torch.equal(y2 != 0, y != 0)                   # fresh counters on the next call
    assert ops.dropout(x, 0.25, False) is x and ops.dropout(x, 0.0, True) is x


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n,offset", [(800 * 32 * 640, 0), (100003, 12345), (7, 3), (1 << 20, (1 << 33) + 5)])
def test_dropout_bit_exact_vs_philox_oracle(dev, p, n, offset):
    """R6: ctcn_dropout(x, p, seed, offset) == x * m / (1 - p) with m drawn by the host restatement of Philox4x32-10
    (oracle/philox.py, pinned to the Random123 known-answer vectors), bit for bit: odd sizes (scalar tail), offsets beyond
    2^32 (the high counter word), a misaligned view (scalar path), and the backward pass regenerating the same mask."""
    from ctc_pytorch_amd import _lib
    from oracle import philox
    L = _lib.lib()
    seed = 0x9E3779B97F4A7C15 ^ n
    rs = np.random.RandomState(n % 9973)
    xh = rs.standard_normal(n + 1).astype(np.float32)
    for shift in (0, 1):                                    # shift 1: 4-byte aligned only -> the kernel's scalar path
        x = torch.from_numpy(xh).to(dev)[shift:shift + n]
        y = torch.empty(n + 1, device=dev)[shift:shift + n]
        _lib.check(L.ctcn_dropout(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), n, p, seed, offset, _lib.stream_ptr()), "dropout")
        want = philox.dropout(xh[shift:shift + n], p, seed, offset)
        got = y.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    # through autograd: forward and backward draw the same mask from the (seed, offset) the wrapper recorded
    from ctc_pytorch_amd import ops
    xg = torch.from_numpy(xh[:n]).to(dev).requires_grad_(True)
    yg = ops.dropout(xg, p, True)
    gy = torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev)
    yg.backward(gy)
    pp, sd, off = yg.grad_fn.rng
    assert np.array_equal(yg.detach().cpu().numpy(), philox.dropout(xh[:n], pp, sd, off))
    assert np.array_equal(xg.grad.cpu().numpy(), philox.dropout(gy.cpu().numpy(), pp, sd, off))


def test_adam_vs_oracle(dev):
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(4)
    n = 10007
    p, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n), np.zeros(n)
    pr = p.astype(np.float64)
    pt, mt, vt = gpu(p, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(1, 4):
        gs = (g * step).astype(np.float32)
        pr, m, v = R.adam_step(pr, gs.astype(np.float64), m, v, step, 1e-3, 5e-4)
        ops.adam_step(pt, gpu(gs, dev), mt, vt, 1e-3, 0.9, 0.999, 1e-8, 5e-4, step)
    assert maxabs(pt, pr) < 2e-6


def test_flat_adam_state_dict_is_the_torch_adam_layout(dev):
    """'optim_dict' of a package must load on either side.  FlatAdam.state_dict() -> torch.optim.Adam.load_state_dict
    and back; after the hand-over both optimisers take the same next step."""
    import copy
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.optim import FlatAdam
    rp = {"rnn_input_size": 40, "rnn_hidden_size": 16, "rnn_layers": 2, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    torch.manual_seed(3)
    m1 = CTC_Model(rnn_param=rp, num_class=12, drop_out=0.0).to(dev)
    m2 = copy.deepcopy(m1)
    fa = FlatAdam(m1, lr=2e-3, weight_decay=5e-4)
    ta = torch.optim.Adam(m2.parameters(), lr=2e-3, weight_decay=5e-4)
    assert fa.state_dict()["state"] == {} and fa.state_dict()["param_groups"][0]["params"] == list(range(len(list(m2.parameters()))))
    gen = torch.Generator(device="cpu").manual_seed(5)
    def fake_grads(model):
        gs = [torch.randn(p.shape, generator=gen) for p in model.parameters()]
        return gs
    for step in range(3):
        gs = fake_grads(m1)
        fa.zero_grad()
        for p, g in zip(m1.parameters(), gs):
            p.grad.copy_(g.to(dev))
        for p, g in zip(m2.parameters(), gs):
            p.grad = g.to(dev)
        fa.step()
        ta.step()
        if step == 0:                                   # hand the moments over in both directions after the first step
            sd_f, sd_t = copy.deepcopy(fa.state_dict()), copy.deepcopy(ta.state_dict())
            assert set(sd_f["param_groups"][0]) == set(sd_t["param_groups"][0]) and set(sd_f["state"]) == set(sd_t["state"])
            ta.load_state_dict(sd_f)
            fa.load_state_dict(sd_t)
            assert fa.step_count == 1
    for (k, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert maxabs(a, b) < 2e-6, k
    legacy = {"step": 3, "m": fa.m.clone(), "v": fa.v.clone(), "layout": list(fa.layout), "param_groups": [{"lr": 1e-4}]}
    fa.load_state_dict(legacy)                          # round-1 packages still load
    assert fa.param_groups[0]["lr"] == 1e-4 and fa.step_count == 3


def test_ctc_rejects_lengths_outside_the_tensors(dev):
    """torch.nn.CTCLoss raises on input_lengths > T / target_lengths > Lmax / negative lengths.  Host-resident
    lengths raise here too; device-resident ones make the kernels return NaN for that utterance (loss and gradient rows)
    without touching memory outside the tensors; the edit-distance kernel clamps."""
    from ctc_pytorch_amd import nn, ops
    T, B, V, Lmax = 20, 3, 8, 5
    rs = np.random.RandomState(0)
    lp = ops.log_softmax(torch.from_numpy(rs.standard_normal((T, B, V)).astype(np.float32)).to(dev)).requires_grad_(True)
    tg = torch.from_numpy(rs.randint(1, V, size=(B, Lmax)).astype(np.int64))
    ok_in, ok_tl = torch.tensor([20, 15, 9]), torch.tensor([5, 3, 2])
    loss_fn = nn.CTCLoss(reduction="sum")
    for bad_in, bad_tl in ((torch.tensor([21, 15, 9]), ok_tl), (ok_in, torch.tensor([6, 3, 2])), (torch.tensor([20, -1, 9]), ok_tl)):
        with pytest.raises(ValueError):
            loss_fn(lp, tg, bad_in, bad_tl)
    nll = nn.CTCLoss(reduction="none")(lp.detach(), tg.to(dev), torch.tensor([21, 15, 9]).to(dev), torch.tensor([5, 7, 2]).to(dev)).cpu().numpy()
    assert np.isnan(nll[0]) and np.isnan(nll[1]) and np.isfinite(nll[2])
    loss = loss_fn(lp, tg.to(dev), torch.tensor([20, 15, 40]).to(dev), ok_tl.to(dev))
    loss.backward()
    g = lp.grad.cpu().numpy()
    assert np.isnan(float(loss)) and np.isnan(g[:, 2]).all() and np.isfinite(g[:, :2]).all()
    ids = torch.from_numpy(rs.randint(1, V, size=(B, T)).astype(np.int32)).to(dev)
    d = ops.edit_distance(ids, torch.tensor([4, 50, -3], dtype=torch.int32, device=dev), tg.to(dev), torch.tensor([5, 99, 2]).to(dev)).cpu().numpy()
    assert d[0] >= 1 and 0 <= d[1] <= T                     # lengths clamped to the buffers: finite, no fault
    assert d[2] == 2


# ---------------------------------------------------------------------------------------------------------
# whole model
# ---------------------------------------------------------------------------------------------------------
def _build_model(tag, dev):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    V = 62
    base = {"rnn_input_size": 121 if "bigbank" in tag else 40, "bidirectional": True, "batch_norm": True, "rnn_layers": 2}
    if tag == "lstm2x32":
        m = CTC_Model(rnn_param=dict(base, rnn_hidden_size=32, rnn_type=nn.LSTM), num_class=V, drop_out=0.0)
    elif tag == "gru2x24":
        m = CTC_Model(rnn_param=dict(base, rnn_hidden_size=24, rnn_type=nn.GRU), num_class=V, drop_out=0.0)
    elif tag == "rnn2x20_uni_nobn":
        m = CTC_Model(rnn_param=dict(base, rnn_hidden_size=20, rnn_type=nn.RNN, bidirectional=False, batch_norm=False),
                      num_class=V, drop_out=0.0)
    else:
        layers = [[(1, 32), (3, 3), (1, 2), (1, 1), None], [(32, 32), (3, 3), (2, 2), (1, 1), None]]
        if tag == "cnn_pool_lstm2x16":           # MaxPool2d over time after each conv block (model_ctc.py:52-53)
            layers = [[(1, 8), (3, 3), (1, 2), (1, 1), (2, 1)], [(8, 8), (3, 3), (1, 2), (1, 1), (3, 1)]]
        if tag == "cnn_bigbank_lstm2x16":        # (round 6) the reference's example front-end, model_ctc.py:232-233: 123 taps; a 258-KB filter bank
            layers = [[(1, 32), (3, 41), (1, 2), (0, 0), None], [(32, 32), (3, 21), (2, 2), (0, 0), None]]
        cnn_param = {"batch_norm": True, "activate_function": nn.ReLU, "layer": layers}
        m = CTC_Model(add_cnn=True, cnn_param=cnn_param, rnn_param=dict(base, rnn_hidden_size=16, rnn_type=nn.LSTM),
                      num_class=V, drop_out=0.0)
    z = load("model_" + tag)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=int(z["seed_w"]))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    return m.to(dev), z


@pytest.mark.parametrize("rnn,H,B,T", [("LSTM", 320, 32, 208), ("GRU", 256, 20, 419), ("LSTM", 128, 16, 1031)])
def test_forward_projection_overlap_equals_inline(dev, rnn, H, B, T):
    """Pipelined input projection (ctcn_rnn_call.side_stream of ctcn_rnn_fwd_ex: only the first pair of time chunks is projected before the persistent
    recurrence starts, the rest on the side stream behind a chunk counter) against the plain order: outputs, saved activations and
    the gradients computed from them are bit-identical, five times in a row (a chunk read before its GEMM landed would show)."""
    from ctc_pytorch_amd import nn, ops
    ops.set_precision(1)
    rs = np.random.RandomState(T)
    layer = getattr(nn, rnn)(40, H, bidirectional=True, bias=False).to(dev)
    x = torch.from_numpy(rs.standard_normal((T, B, 40)).astype(np.float32)).to(dev)
    gy = torch.from_numpy(rs.standard_normal((T, B, 2 * H)).astype(np.float32)).to(dev)
    outs = {}
    try:
        ops.set_option("fwd_pipe_any_chunking", 1)                 # (these shapes have no chunk count that fits the side stream's one-round rule)
        for mode in (False, True, True, True, True, True):
            ops.set_fwd_overlap(mode)
            xin = x.clone().requires_grad_()
            for p_ in layer.parameters():
                p_.grad = None
            y, _ = layer(xin)
            y.backward(gy)
            torch.cuda.synchronize()
            ops.check_health()
            got = [y.detach().clone(), xin.grad.clone()] + [p_.grad.clone() for p_ in layer.parameters()]
            if mode not in outs:
                outs[mode] = got
            else:
                assert all(torch.equal(a, b_) for a, b_ in zip(got, outs[mode]))
    finally:
        ops.set_fwd_overlap(True)
        ops.set_option("fwd_pipe_any_chunking", 0)
    assert all(torch.equal(a, b_) for a, b_ in zip(outs[True], outs[False]))


@pytest.mark.parametrize("T", [57, 50, 43, 36, 58, 64])
@pytest.mark.parametrize("rsv", [1, 0])
def test_forward_projection_overlap_short_last_chunk(dev, T, rsv):
    """with 8 time chunks and T = 36 / 43 / 50 / 57 the last chunk holds ONE frame, so step 1 of the reverse direction
    (frame T - 2) lies in chunk pair 1, which the side stream projects after the recurrence was launched -- and the prologue of the
    reserve-through-LDS variant (`fwd_rsv_lds = 1`) fetches the pre-activations of steps 0 and 1 without looking at the chunk counter.
    The host now keeps such a T off the pipeline; with the side-stream threshold lowered so that the pipeline WOULD apply, output,
    reserves-derived gradients and weight gradients equal the inline order bit for bit, six runs in a row."""
    from ctc_pytorch_amd import nn, ops
    ops.set_precision(1)
    H, B = 320, 32
    rs = np.random.RandomState(T)
    layer = nn.LSTM(40, H, bidirectional=True, bias=False).to(dev)
    x = torch.from_numpy(rs.standard_normal((T, B, 40)).astype(np.float32)).to(dev)
    gy = torch.from_numpy(rs.standard_normal((T, B, 2 * H)).astype(np.float32)).to(dev)
    outs = {}
    old_min, old_min_bwd = ops._side["min_items"], ops._side["min_items_bwd"]
    try:
        ops.set_side_stream(True, min_items=1)
        ops.set_option("fwd_pipe_any_chunking", 1)
        ops.set_option("fwd_rsv_lds", rsv)
        for mode in (False, True, True, True, True, True, True):
            ops.set_fwd_overlap(mode)
            xin = x.clone().requires_grad_()
            for p_ in layer.parameters():
                p_.grad = None
            y, _ = layer(xin)
            y.backward(gy)
            torch.cuda.synchronize()
            ops.check_health()
            assert ops.rnn_last_kernels()[0] == "rnn_fwd_tagged"
            got = [y.detach().clone(), xin.grad.clone()] + [p_.grad.clone() for p_ in layer.parameters()]
            if mode not in outs:
                outs[mode] = got
            else:
                assert all(torch.equal(a, b_) for a, b_ in zip(got, outs[mode]))
    finally:
        ops.set_fwd_overlap(True)
        ops.set_option("fwd_pipe_any_chunking", 0)
        ops.set_option("fwd_rsv_lds", 2)
        ops.set_side_stream(True, min_items=old_min, min_items_bwd=old_min_bwd)
    assert all(torch.equal(a, b_) for a, b_ in zip(outs[True], outs[False]))


@pytest.mark.parametrize("rnn,H,B,T,I,bidir", [("LSTM", 320, 32, 100, 640, True), ("GRU", 256, 20, 77, 40, True), ("LSTM", 64, 5, 33, 24, False),
                                               ("LSTM", 24, 3, 9, 8, True), ("RNN", 32, 4, 12, 8, True), ("LSTM", 30, 2, 7, 6, True)])
def test_rnn_layer_with_fused_dropout_equals_layer_then_dropout(dev, rnn, H, B, T, I, bidir):
    """BatchRNN's `dropout(rnn(x))` in one call (ctcn_rnn_fwd_dropout): where the tagged-gather recurrence applies the dropped output is
    stored by the recurrence itself (Philox in the item waves), elsewhere -- other kernels, hidden sizes that are padded -- a dropout pass
    follows; in every case output, input gradient and weight gradients are bit-identical to the layer followed by ops.dropout with the
    same position in the random stream, at both matmul precisions."""
    from ctc_pytorch_amd import nn, ops
    rs = np.random.RandomState(H + T)
    layer = getattr(nn, rnn)(I, H, bidirectional=bidir, bias=False).to(dev).train()
    x = torch.from_numpy(rs.standard_normal((T, B, I)).astype(np.float32)).to(dev)
    D = 2 if bidir else 1
    gy = torch.from_numpy(rs.standard_normal((T, B, D * H)).astype(np.float32)).to(dev)
    for prec in (1, 0):
        ops.set_precision(prec)
        outs = []
        try:
            for mode in ("separate", "fused", "fused_kernel_off"):
                ops.set_option("rnn_fused_dropout", 0 if mode == "fused_kernel_off" else 1)
                ops._drop_counter[0] = 1000                       # the same position in the Philox stream for every mode
                torch.manual_seed(5)
                xin = x.clone().requires_grad_()
                for p_ in layer.parameters():
                    p_.grad = None
                if mode == "separate":
                    y, _ = layer(xin)
                    y = ops.dropout(y, 0.25, True)
                else:
                    y, _ = layer(xin, drop_p=0.25)
                y.backward(gy)
                torch.cuda.synchronize()
                ops.check_health()
                outs.append([y.detach().clone(), xin.grad.clone()] + [p_.grad.clone() for p_ in layer.parameters()])
                assert ops._drop_counter[0] == 1000 + (y.numel() + 3) // 4
        finally:
            ops.set_option("rnn_fused_dropout", 1)
            ops.set_precision(0)
        kept = float((outs[0][0] != 0).float().mean())
        assert 0.6 < kept < 0.9
        for o in outs[1:]:
            assert all(torch.equal(a, b_) for a, b_ in zip(o, outs[0]))


def test_rnn_abi_is_stateless_two_layers_two_streams_two_threads(dev):
    """no hidden state behind the C ABI.  Two recurrent layers (different shapes, different dropout streams, their
    own status words) are driven through ctcn_rnn_fwd_ex / ctcn_rnn_bwd_ex from two host THREADS on two HIP streams at the same time, many
    times over; every result must equal the one the same call produces alone.  (Before round 3 the dropout request, the projection
    pipeline and the pre-launch event travelled in thread-locals armed by separate setter calls.)"""
    import threading
    from ctc_pytorch_amd import _lib, ops
    L = _lib.lib()
    ops.set_precision(1)

    class Layer:
        def __init__(self, seed, T, B, I, H, cell, p):
            g = torch.Generator(device="cpu").manual_seed(seed)
            G = {0: 4, 1: 3}[cell]
            self.dims, self.cell, self.p, self.seed = (T, B, I, H), cell, p, seed
            self.x = (torch.randn(T, B, I, generator=g) * 0.5).to(dev)
            self.w = (torch.randn(2 * G * H, I, generator=g) * 0.1).to(dev)          # [W_ih fwd ; W_ih rev] stacked
            self.u = [(torch.randn(G * H, H, generator=g) * 0.1).to(dev) for _ in range(2)]
            self.gy = torch.randn(T, B, 2 * H, generator=g).to(dev)
            self.stream = torch.cuda.Stream(device=dev)
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self.ws = torch.empty(256 << 20, dtype=torch.uint8, device=dev)

        def run(self):
            T, B, I, H = self.dims
            G = {0: 4, 1: 3}[self.cell]
            with torch.cuda.stream(self.stream):
                y, yd = torch.empty(T, B, 2 * H, device=dev), torch.empty(T, B, 2 * H, device=dev)
                gates, aux = torch.empty(T, B, 2, G * H, device=dev), torch.empty(T, B, 2, H, device=dev)
                call = _lib.RnnCall()
                call.status, call.y_drop, call.drop_p, call.drop_seed, call.drop_offset = self.status.data_ptr(), yd.data_ptr(), self.p, self.seed, 1000 * self.seed
                st = ctypes.c_void_p(self.stream.cuda_stream)
                wp = ctypes.c_void_p(self.ws.data_ptr())
                P = lambda t: ctypes.c_void_p(t.data_ptr())
                w1 = self.w[G * H:]
                _lib.check(L.ctcn_rnn_fwd_ex(self.cell, T, B, I, H, 2, P(self.x), P(self.w), P(self.u[0]), P(w1), P(self.u[1]), P(y), P(gates), P(aux), 1,
                                             wp, self.ws.numel(), st, ctypes.byref(call)), "rnn_fwd_ex")
                dx, gd = torch.empty_like(self.x), torch.empty_like(self.gy)
                dw = [torch.empty(G * H, I, device=dev), torch.empty(G * H, H, device=dev), torch.empty(G * H, I, device=dev), torch.empty(G * H, H, device=dev)]
                scratch = torch.empty(L.ctcn_rnn_scratch_bytes(self.cell, B, H, 2), dtype=torch.uint8, device=dev)
                call2 = _lib.RnnCall()
                call2.status, call2.dy_tmp, call2.drop_p, call2.drop_seed, call2.drop_offset = self.status.data_ptr(), gd.data_ptr(), self.p, self.seed, 1000 * self.seed
                _lib.check(L.ctcn_rnn_bwd_ex(self.cell, T, B, I, H, 2, P(self.x), P(self.w), P(self.u[0]), P(w1), P(self.u[1]), P(y), P(gates), P(aux), P(self.gy),
                                             P(dx), P(dw[0]), P(dw[1]), P(dw[2]), P(dw[3]), 0.0, 1, P(scratch), wp, self.ws.numel(), st, ctypes.byref(call2)), "rnn_bwd_ex")
                self.stream.synchronize()
            return [t.clone() for t in (y, yd, dx, dw[0], dw[1], dw[2], dw[3])]

    a, b = Layer(3, 70, 32, 48, 320, 0, 0.1), Layer(5, 45, 20, 64, 128, 1, 0.3)
    ref_a, ref_b = a.run(), b.run()                      # each alone
    assert float(ref_a[1].eq(0).float().mean()) > 0.05 and float(ref_b[1].eq(0).float().mean()) > 0.2      # the dropout really ran, at its own p
    errs = []

    def worker(layer, ref):
        try:
            for _ in range(12):
                got = layer.run()
                for g_, r_ in zip(got, ref):
                    if not torch.equal(g_, r_):
                        errs.append("mismatch")
        except Exception as e:                       # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(a, ref_a)), threading.Thread(target=worker, args=(b, ref_b))]
    [t.start() for t in th]
    [t.join() for t in th]
    torch.cuda.synchronize()
    assert not errs, errs[:3]
    assert int(a.status.item()) == 0 and int(b.status.item()) == 0


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("rnn,H,B,T", [("LSTM", 128, 8, 60), ("GRU", 192, 40, 25), ("LSTM", 96, 64, 30)])      # (B = 64: no idle XCD -- the free CUs next to the recurrence, every XCD)
def test_weight_gradient_side_stream_equals_inline(dev, rnn, H, B, T, prec):
    """FlatAdam, both matmul precisions: the weight-gradient GEMMs run on the second stream, restricted to the XCDs the next
    layer's persistent recurrence leaves idle (queue kernels), and are joined when backward ends.  Same flat gradient,
    bit for bit, as the inline path (same tiles, same split-K order), also over two accumulating backward passes."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.optim import FlatAdam
    V = 30
    m = CTC_Model(rnn_param={"rnn_input_size": 40, "bidirectional": True, "batch_norm": True, "rnn_layers": 3, "rnn_hidden_size": H,
                             "rnn_type": getattr(nn, rnn)}, num_class=V, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=5)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    m = m.to(dev).train()
    opt = FlatAdam(m, lr=1e-3)
    b = synth.make_batch(seed=21, B=B, T=T, F=40, V=V, lab_lo=3, lab_hi=8)
    x, tg, tl = gpu(b["x"], dev), gpu(b["targets"], dev), gpu(b["tgt_len"], dev)
    il = torch.full((B,), T, dtype=torch.int64, device=dev)
    loss_fn = nn.CTCLoss(reduction="sum")
    flat = next(p for p in m.parameters())._ctcn_grad
    base = flat.untyped_storage()
    grads = {}
    ops.set_precision(prec)
    try:
        for side in (False, True):
            ops.set_side_stream(side, min_items=0)         # the layers of this test are below the default size threshold
            opt.zero_grad()
            for _ in range(2):                              # gradients accumulate (beta = 1) across backward passes
                loss = loss_fn(m(x), tg, il, tl) / B
                loss.backward()
            torch.cuda.synchronize()
            grads[side] = torch.cat([p._ctcn_grad.reshape(-1) for p in m.parameters()]).clone()
    finally:
        ops.set_precision(0)
        ops.set_side_stream(True, min_items=ops.SIDE_MIN_ITEMS_FWD, min_items_bwd=ops.SIDE_MIN_ITEMS_BWD)
    ops.check_health()
    assert base is not None and torch.isfinite(grads[True]).all()
    assert float(grads[True].abs().max()) > 0
    assert torch.equal(grads[True], grads[False])


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("tag", ["lstm2x32", "gru2x24", "rnn2x20_uni_nobn", "cnn_lstm2x16", "cnn_pool_lstm2x16", "cnn_bigbank_lstm2x16"])
@pytest.mark.parametrize("flat", [True, False])
def test_model_three_steps_golden(dev, tag, flat, prec):
    """Whole-model fixtures captured from the reference (oracle/gen_golden.py): `visualize` activations, log-probs, arg-max,
    all parameter gradients, 3 Adam steps, eval forward -- at both matmul precisions.  precision 0: the f32-strict gates;
    precision 1 (the library default, the mode bench.py measures): SURVEY 8a's bf16-mode gates."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.optim import FlatAdam
    ops.set_precision(prec)
    tol_act, tol_grad, tol_loss = gates(prec, 5e-5, 2e-4, 2e-5)
    m, z = _build_model(tag, dev)
    m.train()
    x, tg, tl = gpu(z["x"], dev), gpu(z["targets"], dev), gpu(z["tgt_len"], dev)
    B = x.shape[0]
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4) if flat else torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
    loss_fn = nn.CTCLoss(reduction="sum")
    losses = []
    for step in range(3):
        lp, vis = m(x, visualize=True)
        in_len = torch.from_numpy(R.frames_from_fraction(z["frac"], lp.size(0)))
        if step == 0:
            assert np.array_equal(in_len.numpy(), z["in_len"])
            assert maxabs(lp, z["lp"]) < tol_act
            argmax_report(lp, z["argmax"], tag)
            if "rnn_in" in z.files:
                assert maxabs(vis[1], z["conv_out"]) < tol_act and maxabs(vis[2], z["rnn_in"]) < tol_act
        loss = loss_fn(lp, tg, in_len.to(dev), tl) / B
        opt.zero_grad()
        loss.backward()
        if step == 0:
            for k, p in m.named_parameters():
                if k.endswith("conv.bias"):
                    # a bias feeding BatchNorm has an identically-zero gradient in exact arithmetic: both sides hold
                    # float32 rounding noise (reference ~1e-6), so only its magnitude is checked
                    assert float(p.grad.abs().max()) < 1e-4, k
                    continue
                assert rel_l2(p.grad, z["g." + k]) < tol_grad or maxabs(p.grad, z["g." + k]) < 1e-6, k
        opt.step()
        losses.append(float(loss))
    assert np.allclose(losses, z["losses"], rtol=tol_loss), (losses, z["losses"])
    for k, v in m.state_dict().items():
        want = z["after." + k]
        if "num_batches" in k:
            assert int(v) == int(want), k
        elif k.endswith("conv.bias") or (k.startswith("conv.") and k.endswith("running_mean")):
            # the bias gradient is pure rounding noise (see above) and Adam normalises noise to +-lr per step; the
            # BatchNorm running mean right after the conv inherits that drift (0.1 * bias difference per step)
            assert maxabs(v, want) < 3.5e-3, k
        else:
            # Adam turns a gradient into lr*sign-like steps, so an entry whose gradient is smaller than the float32
            # rounding noise of its tensor (measured: |g| ~ 2e-5 against ~5e-5 of noise in rnns.1.rnn.weight_hh_l0 of the
            # CNN model, both sides; tools/dbg_cnn.py shows every per-step gradient within 4e-5 rel-L2 of torch) can move
            # by +-lr per step in either implementation.  Gate: (almost) all entries within 5e-5, none beyond 3 steps * lr;
            # precision 1 additionally: rel-L2 of the whole tensor within the bf16-mode gate.
            dv = (v.detach().cpu().double() - torch.from_numpy(np.asarray(want)).double()).abs()
            assert float(dv.max()) < 3.5e-3, k
            if prec == 0:
                assert float((dv > 5e-5).double().mean()) < 0.01, (k, float(dv.max()))
            else:
                assert rel_l2(v, want) < tol_grad or float(dv.max()) < 1e-5, (k, rel_l2(v, want))
    m.eval()
    with torch.no_grad():
        lpe = m(x)
    assert maxabs(lpe, z["lp_eval_after"]) < (2e-4 if prec == 0 else tol_act)
    argmax_report(lpe, z["argmax_eval_after"], tag + " (eval, after 3 steps)")


@pytest.mark.parametrize("prec", [0, 1])
def test_run_epoch_trajectory_golden(dev, prec):
    """cfg1 (2x128 BiLSTM, B=8, T=300, full size): the reference's printed 3-step loss trajectory, (acc, avg loss) returns of a
    train epoch and of an eval epoch -- error counts identical, losses to 1e-4 (f32-strict) / 1e-3 (bf16 mode)."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    ops.set_precision(prec)
    rt = 1e-4 if prec == 0 else 1e-3
    from ctc_pytorch_amd.optim import FlatAdam
    from ctc_pytorch_amd.steps.train_ctc import run_epoch
    z = load("run_epoch_cfg1")
    rp = {"rnn_input_size": 40, "rnn_hidden_size": 128, "rnn_layers": 2, "rnn_type": nn.LSTM, "bidirectional": True,
          "batch_norm": True}
    m = CTC_Model(rnn_param=rp, num_class=62, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=int(z["seed_w"]))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    m = m.to(dev)
    batch = (torch.from_numpy(z["x"]), torch.from_numpy(z["frac"]), torch.from_numpy(z["targets"]),
             torch.from_numpy(z["tgt_len"]), ["u%d" % i for i in range(8)])
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4)
    lines = []
    acc, avg = run_epoch(1, m, [batch, batch, batch], nn.CTCLoss(reduction="sum"), dev, optimizer=opt, print_every=1,
                         is_training=True, log=lines.append)
    step_losses = [float(l.split("cur_loss = ")[1].split(",")[0]) for l in lines if "cur_loss" in l]
    assert np.allclose(step_losses, z["printed_step_losses"], rtol=rt), (step_losses, z["printed_step_losses"])
    assert abs(avg - float(z["train_avg_loss"])) / float(z["train_avg_loss"]) < rt
    # error counts: identical in f32.  In the bf16 mode an untrained model (near-uniform posteriors) has frames whose two best
    # classes are closer than the 1e-5 the modes differ by; SURVEY 8a: report the margin.  Gate: at most 3 greedy errors of the
    # ~1 000 scored tokens differ, and (below) every arg-max flip of the initial model is a near-tie (f32 top-2 margin < 1e-4).
    tokens = float(np.sum(z["tgt_len"]))
    slack = 1e-9 if prec == 0 else 3.0 / (3 * tokens)
    assert abs(acc - float(z["train_acc"])) < slack, (acc, float(z["train_acc"]))
    acc_e, avg_e = run_epoch(1, m, [batch], nn.CTCLoss(reduction="sum"), dev, optimizer=None, is_training=False, log=lines.append)
    assert abs(avg_e - float(z["eval_avg_loss"])) / float(z["eval_avg_loss"]) < (2e-4 if prec == 0 else rt)
    assert abs(acc_e - float(z["eval_acc"])) < (1e-9 if prec == 0 else 3.0 / tokens), (acc_e, float(z["eval_acc"]))
    if prec == 1:
        lps = {}
        for pr in (0, 1):
            ops.set_precision(pr)
            m0 = CTC_Model(rnn_param=rp, num_class=62, drop_out=0.0)
            m0.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
            with torch.no_grad():
                lps[pr] = m0.to(dev).train()(batch[0].to(dev))
        a0, a1 = ops.argmax_last(lps[0]), ops.argmax_last(lps[1])
        flips = a0 != a1
        if bool(flips.any()):
            top2 = torch.topk(lps[0][flips], 2, dim=-1).values
            assert float((top2[:, 0] - top2[:, 1]).max()) < 1e-4, (int(flips.sum()), float((top2[:, 0] - top2[:, 1]).max()))


def _full_size_model(name, dev):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    shapes = json.load(open(os.path.join(G, "large_checksums.json")))
    c = dict(B=8, T=300, V=62, H=128, L=2, rnn="LSTM", cnn=False) if name == "cfg1" else shapes[name]["shape"]
    lab = c.get("lab") or ((60, 100) if name.startswith("cfg4") else ((10, 35) if name == "cfg1" else (30, 60)))
    Fd = c.get("F", 40)                      # ref_yaml: the shipped timit/conf/ctc_config.yaml shape (243-d spliced input)
    b = synth.make_batch(seed=1, B=c["B"], T=c["T"], F=Fd, V=c["V"], lab_lo=lab[0], lab_hi=lab[1])
    rp = {"rnn_input_size": Fd, "rnn_hidden_size": c["H"], "rnn_layers": c["L"], "rnn_type": getattr(nn, c["rnn"]),
          "bidirectional": True, "batch_norm": True}
    if c["cnn"]:
        cp = {"batch_norm": True, "activate_function": nn.ReLU,
              "layer": [[(1, 32), (3, 3), (1, 2), (1, 1), None], [(32, 32), (3, 3), (2, 2), (1, 1), None]]}
        m = CTC_Model(add_cnn=True, cnn_param=cp, rnn_param=rp, num_class=c["V"], drop_out=0.0)
    else:
        m = CTC_Model(rnn_param=rp, num_class=c["V"], drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=91)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    return m.to(dev).train(), b, c


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4"])
def test_full_size_bf16x3_against_f32_vectors(dev, name):
    """The benchmarked arithmetic (precision 1) against the exact-f32 HIP path (precision 0, itself held to the reference's
    checksums below and to the small fixtures) at the FULL BASELINE shapes, vector by vector -- what norms cannot show:
    log-probs max-abs <= 1e-3, loss rel <= 1e-3, every parameter gradient rel-L2 <= 1e-3 (SURVEY 8a bf16-mode gates);
    arg-max identical except on frames whose f32 top-2 margin is below 1e-4 (near-ties; count and margins reported)."""
    from ctc_pytorch_amd import nn, ops
    runs = {}
    for prec in (0, 1):
        ops.set_precision(prec)
        m, b, c = _full_size_model(name, dev)
        lp = m(gpu(b["x"], dev))
        in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0))).to(dev)
        loss = nn.CTCLoss(reduction="sum")(lp, gpu(b["targets"], dev), in_len, gpu(b["tgt_len"], dev)) / c["B"]
        loss.backward()
        torch.cuda.synchronize()
        ops.check_health()
        runs[prec] = (lp.detach(), float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, ops.argmax_last(lp))
    lp0, l0, g0, a0 = runs[0]
    lp1, l1, g1, a1 = runs[1]
    assert maxabs(lp1, lp0) < 1e-3, maxabs(lp1, lp0)
    assert abs(l1 - l0) / abs(l0) < 1e-3
    worst = max((rel_l2(g1[k], g0[k]), k) for k in g0 if not k.endswith("conv.bias"))
    assert worst[0] < 1e-3, worst
    flips = (a0 != a1)
    if bool(flips.any()):
        top2 = torch.topk(lp0[flips], 2, dim=-1).values
        margin = (top2[:, 0] - top2[:, 1])
        assert float(margin.max()) < 1e-4, (int(flips.sum()), float(margin.max()))
        assert int(flips.sum()) <= max(4, a0.numel() // 1000), int(flips.sum())


@pytest.mark.parametrize("prec", [0, 1])
def test_shipped_yaml_model_three_steps_golden(dev, prec):
    """the reference's SHIPPED configuration (timit/conf/ctc_config.yaml:11-40): 243-d spliced input -> 2-layer CNN ->
    61 x 32 = 1 952-wide RNN input (K not a multiple of 64) -> 4 x 384 BiLSTM (the largest hidden size on the scatter path) -> 41 classes.
    Fixture captured from the reference at B = 3, T = 47 (model_ref_yaml.npz): log-probs / arg-max, three Adam steps' losses, norm and a
    strided sample (every 1 009th element) of every gradient and of every updated parameter, eval log-probs after the steps."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.optim import FlatAdam
    ops.set_precision(prec)
    z = load("model_ref_yaml")
    tol_act, tol_grad, tol_loss = gates(prec, 2e-5, 2e-4, 2e-5)
    rp = {"rnn_input_size": 243, "rnn_hidden_size": 384, "rnn_layers": 4, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    cp = {"batch_norm": True, "activate_function": nn.ReLU, "layer": [[(1, 32), (3, 3), (1, 2), (1, 1), None], [(32, 32), (3, 3), (2, 2), (1, 1), None]]}
    m = CTC_Model(add_cnn=True, cnn_param=cp, rnn_param=rp, num_class=41, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=int(z["seed_w"]))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    m = m.to(dev).train()
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4)
    x, tg, tl = gpu(z["x"], dev), gpu(z["targets"], dev), gpu(z["tgt_len"], dev)
    stride = int(z["sample_stride"])
    losses = []
    for step in range(3):
        lp, vis = m(x, visualize=True)
        in_len = torch.from_numpy(R.frames_from_fraction(z["frac"], lp.size(0)))
        if step == 0:
            assert np.array_equal(in_len.numpy(), z["in_len"]) and tuple(vis[2].shape) == tuple(z["rnn_in_shape"])
            assert maxabs(vis[2].reshape(-1)[::stride], z["rnn_in_sample"]) < tol_act
            assert maxabs(lp, z["lp"]) < tol_act, maxabs(lp, z["lp"])
            argmax_report(lp, z["argmax"], "ref_yaml")
        loss = nn.CTCLoss(reduction="sum")(lp, tg, in_len.to(dev), tl) / x.shape[0]
        opt.zero_grad()
        loss.backward()
        if step == 0:
            for k, p in m.named_parameters():
                if k.endswith("conv.bias"):
                    assert float(p.grad.abs().max()) < 1e-4, k
                    continue
                gn = float(p.grad.double().norm())
                assert abs(gn - float(z["gnorm." + k])) <= tol_grad * float(z["gnorm." + k]) + 1e-7, (k, gn, float(z["gnorm." + k]))
                gs, ws = p.grad.reshape(-1)[::stride], z["gsample." + k]
                assert rel_l2(gs, ws) < 5 * tol_grad or maxabs(gs, ws) < 1e-6, (k, rel_l2(gs, ws))
        opt.step()
        losses.append(float(loss))
    ops.check_health()
    assert np.allclose(losses, z["losses"], rtol=max(tol_loss, 5e-5)), (losses, z["losses"])
    m.eval()
    with torch.no_grad():
        lpe = m(x)
    assert maxabs(lpe, z["lp_eval_after"]) < (5e-4 if prec == 0 else 2e-3), maxabs(lpe, z["lp_eval_after"])


_ORACLE_RUNS = {}


def _oracle_full_size(name):
    """One forward / CTC / backward of the torch-CPU oracle (oracle/torch_cpu.py: the reference's own torch calls, pinned against the
    reference fixtures by the CPU suite) at a full BASELINE shape, from the same seeded state dict and batch as _full_size_model.
    Runs once per config and session on the host cores (cfg2 ~3 s)."""
    if name in _ORACLE_RUNS:
        return _ORACLE_RUNS[name]
    shapes = json.load(open(os.path.join(G, "large_checksums.json")))
    c = dict(B=8, T=300, V=62, H=128, L=2, rnn="LSTM", cnn=False) if name == "cfg1" else shapes[name]["shape"]
    lab = c.get("lab") or ((60, 100) if name == "cfg4" else ((10, 35) if name == "cfg1" else (30, 60)))
    Fd = c.get("F", 40)
    b = synth.make_batch(seed=1, B=c["B"], T=c["T"], F=Fd, V=c["V"], lab_lo=lab[0], lab_hi=lab[1])
    rp = {"rnn_input_size": Fd, "rnn_hidden_size": c["H"], "rnn_layers": c["L"], "rnn_type": getattr(tnn, c["rnn"]), "bidirectional": True,
          "batch_norm": True}
    cp = {"batch_norm": True, "activate_function": tnn.ReLU,
          "layer": [[(1, 32), (3, 3), (1, 2), (1, 1), None], [(32, 32), (3, 3), (2, 2), (1, 1), None]]} if c["cnn"] else None
    ref = torch_cpu.TorchCpuCTCModel(add_cnn=c["cnn"], cnn_param=cp, rnn_param=rp, num_class=c["V"], drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], seed=91)
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    ref.train()
    before = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    try:
        lp = ref(torch.from_numpy(b["x"]))
        in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0)))
        loss = tnn.CTCLoss(reduction="sum")(lp, torch.from_numpy(b["targets"]), in_len, torch.from_numpy(b["tgt_len"])) / c["B"]
        loss.backward()
        out = dict(lp=lp.detach(), loss=float(loss), grads={k: p.grad.detach().clone() for k, p in ref.named_parameters()},
                   argmax=R.argmax_first(lp.detach().numpy()))
        # the same torch calls in float64: the yardstick for what "f32-exact" can mean at this depth -- the float32 oracle's OWN distance
        # from it is the rounding floor of an 800-1 200-step recurrence (summation order, 1-ulp transcendentals), not an error of either side
        ref64 = torch_cpu.TorchCpuCTCModel(add_cnn=c["cnn"], cnn_param=cp, rnn_param=rp, num_class=c["V"], drop_out=0.0).double()
        ref64.load_state_dict({k: torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v))
                               for k, v in vals.items()})
        ref64.train()
        lp64 = ref64(torch.from_numpy(b["x"]).double())
        loss64 = tnn.CTCLoss(reduction="sum")(lp64, torch.from_numpy(b["targets"]), in_len, torch.from_numpy(b["tgt_len"])) / c["B"]
        loss64.backward()
        out["lp64"], out["loss64"] = lp64.detach(), float(loss64)
        out["grads64"] = {k: p.grad.detach().clone() for k, p in ref64.named_parameters()}
    finally:
        torch.set_num_threads(before)
    _ORACLE_RUNS[name] = out
    return out


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "ref_yaml"])
def test_full_size_elementwise_vs_torch_cpu_oracle(dev, name, prec):
    """the BASELINE shapes against the ORACLE, vector by vector (norms cannot see a permuted or sign-symmetric error
    inside a 1 280 x 640 gradient): log-probs max-abs, arg-max identical (near-ties reported with their margins), loss, and EVERY
    parameter gradient rel-L2, at both matmul precisions (cfg4 at B = 8, one data-parallel shard, as in the checksum fixture).
    Gates: precision 1 = SURVEY 8a's bf16-mode column (1e-3 everywhere); precision 0 = the measured floor of the f32 path against
    torch CPU at these depths (hardware exp / rcp in 800-1 200 chained gate evaluations, MFMA summation order)."""
    from ctc_pytorch_amd import nn, ops
    want = _oracle_full_size(name)
    ops.set_precision(prec)
    m, b, c = _full_size_model(name, dev)
    lp = m(gpu(b["x"], dev))
    in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0))).to(dev)
    loss = nn.CTCLoss(reduction="sum")(lp, gpu(b["targets"], dev), in_len, gpu(b["tgt_len"], dev)) / c["B"]
    loss.backward()
    torch.cuda.synchronize()
    ops.check_health()
    # no silent fall-back to one launch per timestep at these shapes (H = 384 of ref_yaml is the largest hidden size on the scatter path)
    assert ops.rnn_last_kernels()[0] in ("rnn_fwd_tagged", "rnn_fwd_persist") and ops.rnn_last_kernels()[1] in ("rnn_bwd_scatter2", "rnn_bwd_scatter", "rnn_bwd_persist"), ops.rnn_last_kernels()
    tol_act, tol_grad, tol_loss = gates(prec, 2e-5, 4e-4, 1e-5)
    e_lp = maxabs(lp, want["lp"])
    e_loss = abs(float(loss) - want["loss"]) / abs(want["loss"])
    errs = {k: rel_l2(p.grad, want["grads"][k]) for k, p in m.named_parameters() if not k.endswith("conv.bias")}
    worst = max((v, k) for k, v in errs.items())
    # against the float64 yardstick: the HIP path's distance and the float32 oracle's own distance, per parameter
    ours64 = {k: rel_l2(p.grad.double(), want["grads64"][k]) for k, p in m.named_parameters() if not k.endswith("conv.bias")}
    orac64 = {k: rel_l2(want["grads"][k].double(), want["grads64"][k]) for k in ours64}
    ratio = max((ours64[k] / max(orac64[k], 1e-7), k) for k in ours64)
    e_lp64, o_lp64 = maxabs(lp.double(), want["lp64"]), maxabs(want["lp"].double(), want["lp64"])
    print("\n[%s prec %d] vs f32 oracle: max|dlp| %.3e  loss rel %.3e  grad rel-L2 worst %.3e (%s) median %.3e | vs f64: max|dlp| ours %.3e oracle-f32 %.3e; "
          "grad rel-L2 median ours %.3e oracle-f32 %.3e, worst ratio ours/oracle %.2f (%s)" % (
              name, prec, e_lp, e_loss, worst[0], worst[1], float(np.median(list(errs.values()))), e_lp64, o_lp64,
              float(np.median(list(ours64.values()))), float(np.median(list(orac64.values()))), ratio[0], ratio[1]))
    assert e_lp < tol_act, e_lp
    assert e_loss < tol_loss, e_loss
    assert worst[0] < tol_grad, worst
    if prec == 0:
        # f32-strict, as the float64 run defines it: no parameter gradient may be further from the float64 result than 2.5 x the float32
        # ORACLE's own distance (+ 2e-5): the HIP path is an f32 implementation of the same function, not a less accurate one
        bad = [(k, ours64[k], orac64[k]) for k in ours64 if ours64[k] > 2.5 * orac64[k] + 2e-5]
        assert not bad, bad[:4]
        assert e_lp64 < 2.5 * o_lp64 + 5e-6, (e_lp64, o_lp64)
    for k, p in m.named_parameters():
        if k.endswith("conv.bias"):           # identically zero in exact arithmetic (bias -> BatchNorm): rounding noise on both sides
            assert float(p.grad.abs().max()) < 5e-3, k
    got = ops.argmax_last(lp).cpu().numpy()
    flips = got != want["argmax"]
    if flips.any():
        v = want["lp"].numpy()[flips]
        top2 = np.sort(v, axis=-1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
        assert float(margin.max()) < (1e-5 if prec == 0 else 1e-4) and int(flips.sum()) <= max(2, flips.size // 2000), (int(flips.sum()), margin[:8])


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg4", "ref_yaml", "cfg4_b64"])
def test_large_shape_checksums(dev, name, prec):
    """BASELINE.json full-size configs at both matmul precisions: loss / log-prob checksums / per-parameter gradient norms
    captured from the reference (cfg4 at B=8 per rank, as one DP shard, and -- round 5 -- cfg4_b64: the full per-GPU batch of 64 that
    bench.py times, whose launch geometry (8 groups on every XCD, rnn_bwd_scatter2<8,4,1>) the B = 8 shard never reaches); gradient
    norms within 1e-3."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    ops.set_precision(prec)
    want = json.load(open(os.path.join(G, "large_checksums.json")))[name]
    m, b, c = _full_size_model(name, dev)
    assert sum(p.numel() for p in m.parameters()) == want["n_params"]
    lp = m(gpu(b["x"], dev))
    in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0))).to(dev)
    loss = nn.CTCLoss(reduction="sum")(lp, gpu(b["targets"], dev), in_len, gpu(b["tgt_len"], dev)) / c["B"]
    loss.backward()
    assert abs(float(loss) - want["loss"]) / want["loss"] < 1e-4, (float(loss), want["loss"])
    assert abs(float(lp.double().abs().mean()) - want["lp_abs_mean"]) / want["lp_abs_mean"] < 1e-4
    for k, p in m.named_parameters():
        gn = float(p.grad.double().norm())
        if k.endswith("conv.bias"):        # zero in exact arithmetic (bias -> BatchNorm): rounding noise on both sides
            assert gn < 0.05
            continue
        assert abs(gn - want["grad_norm"][k]) <= 1e-3 * want["grad_norm"][k] + 1e-6, (k, gn, want["grad_norm"][k])
    names = ops.rnn_last_kernels()
    assert "step" not in names[0] + names[1], names          # the persistent recurrences, not one launch per timestep
    if name == "cfg4_b64" and prec == 1:
        assert names == ("rnn_fwd_tagged", "rnn_bwd_scatter2"), names      # the kernels bench.py --workload cfg4 times


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg4_b64"])
def test_bf16_single_mode_against_reference_checksums(dev, name):
    """Option "gemm_bf16_single" (the 256-row GEMM tiles multiply the bf16 roundings of their operands once instead of the three bf16x3
    products): the tolerance BASELINE.json's north_star states -- "CTC loss and LSTM activations within 1e-3 bf16 tolerance" -- on the
    full-size configs against the REFERENCE's checksums: loss and mean |log-prob| within 1e-3 relative (measured: 1e-5 .. 3e-5), every
    parameter's gradient norm within 1 % (measured: 6e-4 .. 4e-3), and the log-probs (magnitude ~4) next to the default mode's on the same
    weights: mean |difference| below 5e-3, none above 5e-2 (measured: 2e-3 .. 3e-3 / 1.8e-2 -- plain bf16 operands carry 8 significant
    bits, so single elements do move in the third digit; the 1e-3 is met by the loss and the averages, not by every element).
    Not the default, not the headline."""
    from ctc_pytorch_amd import nn, ops
    want = json.load(open(os.path.join(G, "large_checksums.json")))[name]
    ops.set_precision(1)
    got = {}
    try:
        for mode in (0, 1):
            ops.set_option("gemm_bf16_single", mode)
            m, b, c = _full_size_model(name, dev)
            lp = m(gpu(b["x"], dev))
            in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0))).to(dev)
            loss = nn.CTCLoss(reduction="sum")(lp, gpu(b["targets"], dev), in_len, gpu(b["tgt_len"], dev)) / c["B"]
            loss.backward()
            got[mode] = (float(loss.detach()), lp.detach().double(), {k: float(p.grad.double().norm()) for k, p in m.named_parameters()})
    finally:
        ops.set_option("gemm_bf16_single", 0)
    loss1, lp1, gn1 = got[1]
    dlp = (lp1 - got[0][1]).abs()
    worst = max(abs(gn1[k] - want["grad_norm"][k]) / want["grad_norm"][k] for k in gn1 if not k.endswith("conv.bias"))
    print("%s: loss %.6f (reference %.6f, rel %.1e)  mean|lp| rel %.1e  |lp - default lp| mean %.1e max %.1e  worst gradient-norm rel %.1e"
          % (name, loss1, want["loss"], abs(loss1 - want["loss"]) / want["loss"],
             abs(float(lp1.abs().mean()) - want["lp_abs_mean"]) / want["lp_abs_mean"], float(dlp.mean()), float(dlp.max()), worst))
    assert abs(loss1 - want["loss"]) / want["loss"] < 1e-3
    assert abs(float(lp1.abs().mean()) - want["lp_abs_mean"]) / want["lp_abs_mean"] < 1e-3
    assert float(dlp.mean()) < 5e-3 and float(dlp.max()) < 5e-2
    assert worst < 1e-2
    assert got[0][0] != loss1                    # (the mode did switch tiles)


# ---------------------------------------------------------------------------------------------------------
# decoders
# ---------------------------------------------------------------------------------------------------------
def test_device_prefetcher_yields_the_loader_batches(dev):
    """async double-buffered H2D staging; same tensors, same order, inputs / length fractions / targets / sizes on
    the device; and the device-side length conversion of run_epoch gives the integers of the host expression."""
    from ctc_pytorch_amd.utils.data_loader import DevicePrefetcher, create_input
    rs = np.random.RandomState(4)
    items = [(torch.from_numpy(rs.standard_normal((int(rs.randint(20, 60)), 40)).astype(np.float32)),
              torch.from_numpy(rs.randint(1, 30, size=int(rs.randint(3, 9))).astype(np.int64)), "utt%d" % i) for i in range(10)]
    batches = [create_input(items[i:i + 4]) for i in range(0, 10, 4)]
    got = list(DevicePrefetcher(batches, dev))
    assert len(got) == len(batches) == 3
    for g, w in zip(got, batches):
        assert all(g[k].device.type == "cuda" for k in range(4))
        assert all(torch.equal(g[k].cpu(), w[k]) for k in range(4))
        assert g[4] == w[4]
        for t_out in (7, 59, 800, 1601):
            assert (g[1].float() * float(t_out)).long().cpu().tolist() == R.frames_from_fraction(w[1].numpy(), t_out).tolist()
    assert list(DevicePrefetcher([], dev)) == []


def test_step_stats_equals_torch(dev):
    """ctcn_step_stats (the four per-step statistics of run_epoch in one launch) against the torch expressions it replaces."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(3)
    for B in (1, 7, 64, 200):
        loss = torch.tensor(rs.rand() * 100, dtype=torch.float32, device=dev)
        dist = torch.from_numpy(rs.randint(0, 90, size=B).astype(np.int32)).to(dev)
        tl = torch.from_numpy(rs.randint(1, 70, size=B).astype(np.int64)).to(dev)
        got = ops.step_stats(loss, dist, tl).cpu().numpy()
        want = np.array([float(loss.double()), float(dist.sum()), float(tl.sum()), 0.0])
        assert np.array_equal(got, want), (B, got, want)


def test_beam_decode_async_two_streams_equals_sync(dev):
    """ops.beam_decode_async (search enqueued on the current stream, results through pinned memory, `result()` waits for that batch alone):
    four batches alternating over two streams -- the way steps/test_ctc.decode_and_score keeps two searches in flight -- return exactly
    what the synchronous call returns for each of them."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    V, T, B, W = 62, 160, 24, 8
    i2c = synth.int2char(V)
    tab = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
    tab_dev = torch.as_tensor(tab, dtype=torch.float64).to(dev)
    xs, lens, want = [], [], []
    for k in range(4):
        lp = synth.make_logprobs(seed=11 + k, T=T, B=B, V=V, regime="peaky" if k % 2 else "flat")
        xs.append(torch.from_numpy(lp).to(dev))
        lens.append(list(np.random.RandomState(k).randint(T // 2, T + 1, size=B)))
        want.append(ops.beam_decode(xs[-1], lens[-1], tab, 0.1, W))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    for _ in range(3):
        handles = []
        for k in range(4):
            with torch.cuda.stream(streams[k % 2]):
                handles.append(ops.beam_decode_async(xs[k], lens[k], tab_dev, 0.1, W))
        for k in (1, 0, 3, 2):                                  # collected out of order
            ids, score, st = handles[k].result()
            assert ids == want[k][0] and np.array_equal(score, want[k][1]) and np.array_equal(st, want[k][2])


def test_end_to_end_train_checkpoint_decode(dev, tmp_path):
    """The reference's workflow on a toy corpus, through the drop-in drivers: Kaldi ark/scp + label + vocab files ->
    steps/train_ctc.main (SpeechDataset, async prefetcher, run_epoch, FlatAdam, LR controller, save_package) ->
    steps/test_ctc.load_package + decode_and_score with the greedy and the LM beam decoder."""
    from ctc_pytorch_amd.steps import test_ctc as TE, train_ctc as TR
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder, GreedyDecoder
    from ctc_pytorch_amd.utils.data_loader import SpeechDataLoader, SpeechDataset, Vocab, write_kaldi_ark
    rs = np.random.RandomState(7)
    phones = ["p%d" % i for i in range(8)]
    proto = rs.standard_normal((len(phones), 40)).astype(np.float32) * 2.0
    mats, labs = {}, {}
    for u in range(24):
        seq = [int(k) for k in rs.randint(0, len(phones), size=int(rs.randint(4, 8)))]
        frames = [proto[k] + 0.3 * rs.standard_normal(40) for k in seq for _ in range(int(rs.randint(5, 9)))]
        mats["utt%02d" % u] = np.asarray(frames, dtype=np.float32)
        labs["utt%02d" % u] = " ".join(phones[k] for k in seq)
    d = str(tmp_path)
    write_kaldi_ark(d + "/feats.ark", d + "/feats.scp", mats)
    open(d + "/text", "w").write("".join("%s %s\n" % kv for kv in labs.items()))
    open(d + "/vocab", "w").write("".join("%d %s\n" % (i, ph) for i, ph in enumerate(phones)))
    synth.write_arpa(d + "/lm.arpa", ["UNK"] + phones, seed=3, n_bigrams=40)
    conf = dict(vocab_file=d + "/vocab", train_scp_path=d + "/feats.scp", train_lab_path=d + "/text", valid_scp_path=d + "/feats.scp",
                valid_lab_path=d + "/text", left_ctx=0, right_ctx=0, n_skip_frame=1, n_downsample=1, batch_size=8, shuffle_train=False,
                num_workers=0, rnn_input_size=40, rnn_hidden_size=32, rnn_layers=2, rnn_type="nn.LSTM", bidirectional=True,
                batch_norm=True, add_cnn=False, layers=2, channel="[(1,32),(32,32)]", kernel_size="[(3,3),(3,3)]", stride="[(1,2),(2,2)]",
                padding="[(1,1),(1,1)]", pooling="None", activation_function="relu", drop_out=0.0, init_lr=1e-2, weight_decay=0.0,
                end_adjust_acc=2.0, lr_decay=0.5, num_epoches=6, verbose_step=100, seed=1, checkpoint_dir=d + "/ckpt", exp_name="toy")
    lines = []
    model, hist = TR.main(conf, log=lines.append)
    assert len(hist["loss"]) == 6 and hist["loss"][-1] < 0.6 * hist["loss"][0], hist["loss"]
    assert hist["dev_acc"][-1] > hist["dev_acc"][0]
    m2, package = TE.load_package(d + "/ckpt/toy/ctc_best_model.pkl", dev)
    assert package["epoch"]["epoch"] == 6 and set(m2.state_dict()) == set(model.state_dict())
    vocab = Vocab(d + "/vocab")

    class O:
        left_ctx = right_ctx = 0
        n_skip_frame = n_downsample = 1
    loader = SpeechDataLoader(SpeechDataset(vocab, d + "/feats.scp", d + "/text", O), batch_size=8, shuffle=False)
    cer_g, wer_g = TE.decode_and_score(m2, loader, GreedyDecoder(vocab.index2word, space_idx=-1, blank_index=0), vocab.index2word, dev, log=lines.append)
    cer_b, wer_b = TE.decode_and_score(m2, loader, BeamDecoder(vocab.index2word, beam_width=5, blank_index=0, space_idx=-1, lm_path=d + "/lm.arpa",
                                                               lm_alpha=0.01), vocab.index2word, dev, log=lines.append)
    assert 0.0 <= wer_g < 100.0 and np.isfinite(cer_g) and np.isfinite(cer_b) and np.isfinite(wer_b)
    # the greedy WER of the scoring script equals 1 - accuracy of the training-time on-device PER at the best epoch
    assert abs(wer_g / 100.0 - (1.0 - max(hist["dev_acc"]))) < 1e-6, (wer_g, hist["dev_acc"])


@pytest.mark.parametrize("wave", [1, 0])
@pytest.mark.parametrize("max_lab", [1, 9, 64, 65, 130, 257, 512, 600])
def test_edit_distance_vs_oracle(dev, wave, max_lab):
    """ctcn_edit_distance (the error count of run_epoch: editdistance.eval at model_ctc.py:200 / ctcDecoder.py:131-149 in the
    reference) against the Levenshtein oracle, bit-exact: the wavefront kernel (anti-diagonals, 1/2/4/8 label columns per lane) and
    the lane-per-utterance kernel, empty predictions and labels, label lengths either side of the 64-column chunk edges, a small
    alphabet (many matches) and a large one."""
    from ctc_pytorch_amd import _lib, ops
    rs = np.random.RandomState(max_lab)
    B, lda = 9, 150
    a = rs.randint(1, 5 if max_lab % 2 else 40, size=(B, lda)).astype(np.int32)
    la = rs.randint(0, lda + 1, size=B).astype(np.int32)
    lb = rs.randint(0, max_lab + 1, size=B).astype(np.int64)
    la[0], lb[0] = 0, max_lab          # empty prediction
    la[1], lb[1] = lda, 0              # empty label
    la[2], lb[2] = 0, 0
    la[3], lb[3] = lda, max_lab
    b = rs.randint(1, 5 if max_lab % 2 else 40, size=(B, max_lab)).astype(np.int64)
    b[4, :min(max_lab, lda)] = a[4, :min(max_lab, lda)]            # a long common prefix
    want = [R.edit_distance(a[u, :la[u]].tolist(), b[u, :lb[u]].tolist()) for u in range(B)]
    _lib.lib().ctcn_set_option(b"edit_wave", wave)
    try:
        got = ops.edit_distance(torch.from_numpy(a).to(dev), torch.from_numpy(la).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(lb).to(dev))
        torch.cuda.synchronize()
    finally:
        _lib.lib().ctcn_set_option(b"edit_wave", 1)
    assert got.cpu().tolist() == want


def test_greedy_decoder_golden(dev):
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.utils.ctcDecoder import GreedyDecoder
    z = load("decoders")
    meta = json.load(open(os.path.join(G, "decoders.json")))
    i2c = synth.int2char(62)
    g = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    for regime in ("peaky", "flat"):
        lp = torch.from_numpy(z["lp_" + regime])            # CPU tensor, as test_ctc.py hands it over
        assert np.array_equal(ops.argmax_last(lp.to(dev)).cpu().numpy(), z["argmax_" + regime].astype(np.int32))
        assert g.decode(lp, meta["lens"]) == meta["greedy_" + regime]
    rp = {"rnn_input_size": 40, "rnn_hidden_size": 4, "rnn_layers": 1, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": False}
    m = CTC_Model(rnn_param=rp, num_class=62, drop_out=0.0).to(dev)
    errs, toks = m.compute_wer(z["argmax_peaky"].T, np.array(meta["lens"]), z["wer_targets"], z["wer_tgt_len"])
    assert [errs, toks] == meta["compute_wer"]
    sc = meta["score_greedy_peaky"]
    dec = g.decode(torch.from_numpy(z["lp_peaky"]), meta["lens"])
    assert sum(g.cer(a, b) for a, b in zip(dec, meta["labels"])) == sc["total_cer"]
    assert sum(g.wer(a, b) for a, b in zip(dec, meta["labels"])) == sc["total_wer"]


def test_beam_decoder_golden(dev):
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    z = load("decoders")
    meta = json.load(open(os.path.join(G, "decoders.json")))
    i2c = synth.int2char(62)
    arpa = os.path.join(G, "lm_phone_bg.arpa")
    bad = []
    for key, want in meta.items():
        if not key.startswith("beam_"):
            continue
        _, regime, w, a = key.split("_")
        bd = BeamDecoder(i2c, beam_width=int(w[1:]), blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=float(a[1:]))
        got = bd.decode(torch.from_numpy(z["lp_" + regime]), meta["lens"])
        if got != want:
            bad.append((key, [i for i in range(len(want)) if got[i] != want[i]]))
    assert not bad, bad
    sc = meta["score_beam_peaky_W5_a0.1"]
    bd = BeamDecoder(i2c, beam_width=5, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.1)
    dec = bd.decode(torch.from_numpy(z["lp_peaky"]), meta["lens"])
    assert sum(bd.cer(a, b) for a, b in zip(dec, meta["labels"])) == sc["total_cer"]


@pytest.mark.parametrize("regime,W", [("peaky", 20), ("flat", 8), ("peaky", 3), ("peaky", 40), ("flat", 33), ("flat", 20), ("peaky", 57)])
def test_beam_vs_c_oracle_random(dev, regime, W):
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    V, T, B = 62, 160, 12
    i2c = synth.int2char(V)
    lp = synth.make_logprobs(seed=101 + W, T=T, B=B, V=V, regime=regime)
    lens = list(np.random.RandomState(5).randint(T // 2, T + 1, size=B))
    tab = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
    lpt = torch.from_numpy(lp)
    probs = torch.exp(lpt)                                  # float32 exp on CPU, as ctcDecoder.py:190
    want, wscore, wst = beam_ref.decode_ids(probs.numpy().transpose(1, 0, 2), lens, tab, 0.1, W)
    got, score, st = ops.beam_decode(probs.to(dev), lens, tab, 0.1, W, 0, input_is_prob=True)
    assert list(st) == list(wst)
    assert got == [list(map(int, s)) for s in want]
    assert np.allclose(score, wscore, rtol=1e-12, atol=1e-12)
    got2, _, _ = ops.beam_decode(lpt.to(dev), lens, tab, 0.1, W, 0, input_is_prob=False)   # device-side exp
    assert got2 == got


@pytest.mark.parametrize("regime", ["peaky", "flat"])
def test_beam_cfg5_full_batch_vs_c_oracle(dev, regime):
    """BASELINE config 5 at full size -- 128 utterances x 800 frames x 62 classes, W = 20, bigram LM, lens U{400..800}, the batch bench.py
    times -- every utterance against the C restatement of BeamSearch.py (bench.py checks 16 + 4 of them).  The flat regime creates up to
    ~15 000 labellings per utterance: past 12 288 the LDS trie is closed and wave 1 goes to the global table, which no smaller test
    reaches.  Labellings and status equal; float64 scores to the last places (ocml vs glibc exp / log)."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    V, T, B, W = 62, 800, 128, 20
    i2c = synth.int2char(V)
    tab = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
    lp = synth.make_logprobs(seed=7, T=T, B=B, V=V, regime=regime)
    lens = list(np.random.RandomState(2).randint(400, 801, size=B))
    probs = torch.exp(torch.from_numpy(lp))
    want, wscore, wst = beam_ref.decode_ids(probs.numpy().transpose(1, 0, 2), lens, tab, 0.1, W)
    got, score, st = ops.beam_decode(probs.to(dev), lens, tab, 0.1, W, 0, input_is_prob=True)      # the same float32 probabilities as the oracle
    assert list(st) == list(wst) and not any(st)
    assert got == [list(map(int, s_)) for s_ in want]
    score, wscore = np.asarray(score), np.asarray(wscore)
    assert np.all(np.abs(score - wscore) <= 4 * np.spacing(np.abs(wscore)))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", [(4, 32, 50 * 20), (3, 8, 37 * 7), (5, 6, 3), (257, 64, 1), (2, 3, 5)])
def test_bn_relu_dropout_fused_equals_two_passes(dev, shape, relu, p):
    """Round 5: BatchNorm (+ ReLU) with the dropout behind it in ONE apply pass (ctcn_bn_fwd_train_dropout / ctcn_bn_bwd_dropout: LayerCNN's
    conv -> BN -> ReLU -> Dropout, model_ctc.py:62-67) against the two passes it replaces -- ops.batch_norm then ops.dropout from the same Philox
    counters: the dropped output, dx, dgamma, dbeta and the running statistics are equal BIT FOR BIT (the keep mask is regenerated from the
    counters, the ReLU mask recomputed from x by the forward's own rounding sequence).  NCHW shapes incl. an inner size that is no multiple of
    four (a Philox group then spans two channels), rows of channels, a tensor whose size is no multiple of four."""
    from ctc_pytorch_amd import ops
    outer, C, inner = shape
    torch.manual_seed(7)
    x0 = torch.randn(outer, C, inner, device=dev) * 1.5 + 0.3
    g0, b0 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
    dy = torch.randn(outer, C, inner, device=dev)
    runs = {}
    for fused in (True, False):
        ops.set_fuse_bn_dropout(fused)
        try:
            ops._drop_counter[0] = 1234
            x = x0.clone().requires_grad_(True)
            g, b = g0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            y = ops.batch_norm(x, g, b, rm, rv, outer, C, inner, True, 0.1, 1e-5, relu, None, drop_p=p)
            y.backward(dy)
            torch.cuda.synchronize()
            runs[fused] = [t.detach().clone() for t in (y, x.grad, g.grad, b.grad, rm, rv)] + [ops._drop_counter[0]]
        finally:
            ops.set_fuse_bn_dropout(True)
    for a, c, name in zip(runs[True], runs[False], ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var", "counter")):
        if name == "counter":
            assert a == c
        else:
            assert torch.equal(a, c), (name, float((a - c).abs().max()))
    if x0.numel() > 5000:
        kept = float((runs[True][0] != 0).float().mean())
        assert abs(kept - (1.0 - p) * (0.5 if relu else 1.0)) < 0.08, kept      # (about half of the activations pass the ReLU)


@pytest.mark.parametrize("regime", ["peaky", "flat"])
@pytest.mark.parametrize("W", [60, 61, 64, 65, 128, 200, 256, 257, 300, 512, 1024])
def test_beam_wide_vs_c_oracle(dev, regime, W):
    """ Beams wider than any earlier test ran: the last width of beam_fast_kernel (60), the first of the generic
    beam_kernel (61), both sides of a 64-lane boundary, 128, the reference's class default 200 (ctcDecoder.py:170), round 5's limit 256 and
    (round 6, VERDICT r5 missing 4: the reference takes any width) 257, 300, 512 and the new BEAM_WMAX = 1 024 -- beam state in dynamic LDS --, on
    the golden batch shape (T = 120, B = 6, ragged lengths) against the C restatement of BeamSearch.py: labellings and status equal,
    float64 scores to the last places."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    V, T, B = 62, 120, 6
    i2c = synth.int2char(V)
    tab = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
    lp = synth.make_logprobs(seed=81 if regime == "peaky" else 82, T=T, B=B, V=V, regime=regime)
    lens = [120, 97, 64, 110, 33, 81]
    if W >= 512:                # (the one-core C oracle needs ~0.1 s per frame at W = 1 024: shorter utterances, the beam still fills)
        lens = [min(l, 40 if W > 512 else 60) for l in lens]
    probs = torch.exp(torch.from_numpy(lp))
    want, wscore, wst = beam_ref.decode_ids(probs.numpy().transpose(1, 0, 2), lens, tab, 0.1, W)
    got, score, st = ops.beam_decode(probs.to(dev), lens, tab, 0.1, W, 0, input_is_prob=True)
    # (a truncated peaky utterance may end with the EMPTY labelling on top -- status 1, the reference's IndexError -- on both sides alike)
    assert list(st) == list(wst) and (W >= 512 or not any(st)) and sum(1 for v in st if v == 0) >= 4
    assert got == [list(map(int, s_)) for s_ in want]
    score, wscore = np.asarray(score), np.asarray(wscore)
    assert np.all(np.abs(score - wscore) <= 4 * np.spacing(np.abs(wscore)))
    # the selection compacts its survivors through an atomic counter and the trie hands out node ids the same way: neither order may show in
    # the results -- a second run returns the same labellings and the same scores bit for bit
    got2, score2, st2 = ops.beam_decode(probs.to(dev), lens, tab, 0.1, W, 0, input_is_prob=True)
    assert got2 == got and np.array_equal(np.asarray(score2), score) and list(st2) == list(st)


@pytest.mark.parametrize("regime", ["peaky", "flat"])
@pytest.mark.parametrize("W,threads,cand_global,bitonic", [(200, 512, 1, 1), (200, 512, 0, 1), (200, 1024, 1, 1), (61, 512, 1, 1), (300, 512, 1, 1), (200, 256, 1, 1),
                                                             (200, 0, 0, 0), (128, 0, 0, 0), (200, 512, 1, 0),
                                                             (257, 256, 0, 1), (300, 256, 0, 1), (513, 512, 0, 1), (600, 512, 0, 1), (1024, 512, 0, 1)])
def test_beam_generic_kernel_occupancy_options(dev, regime, W, threads, cand_global, bitonic):
    """The generic search at other thread counts / candidate-table placements (options beam_generic_threads = 512, beam_cand_global: two
    512-thread searches per CU -- tools/wide_beam_probe.py) and with its survivors ranked by pair counts instead of
    the bitonic sort (beam_bitonic = 0) returns the labellings, status words and float64 scores of the C oracle and, bit for bit, of the
    default configuration.  A forced thread count below W (the kernel gives every beam slot one thread) is raised to the next instantiated
    one: 257 / 300 at 256 threads, 513 / 600 / 1 024 at 512 -- these returned wrong labellings before (slots >= the thread count were never
    merged or materialised).  Those beams fill within three frames at V = 62, so their utterances are cut short: the C oracle's time grows
    with W^2."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    V, T, B = 62, 120, 6
    i2c = synth.int2char(V)
    tab = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
    lp = synth.make_logprobs(seed=83 if regime == "peaky" else 84, T=T, B=B, V=V, regime=regime)
    lens = [120, 97, 64, 110, 33, 81]
    if threads and W > threads:
        cap = 12 if W <= 300 else (8 if W <= 600 else 5)
        lens = [min(l, cap) for l in lens]
    probs = torch.exp(torch.from_numpy(lp))
    want, wscore, wst = beam_ref.decode_ids(probs.numpy().transpose(1, 0, 2), lens, tab, 0.01, W)
    base = ops.beam_decode(probs.to(dev), lens, tab, 0.01, W, 0, input_is_prob=True)
    ops.set_option("beam_generic_threads", threads)
    ops.set_option("beam_cand_global", cand_global)
    ops.set_option("beam_bitonic", bitonic)
    try:
        got, score, st = ops.beam_decode(probs.to(dev), lens, tab, 0.01, W, 0, input_is_prob=True)
    finally:
        ops.set_option("beam_generic_threads", 0)
        ops.set_option("beam_cand_global", 0)
        ops.set_option("beam_bitonic", 1)
    assert list(st) == list(wst) and got == [list(map(int, s_)) for s_ in want]
    assert np.all(np.abs(np.asarray(score) - np.asarray(wscore)) <= 4 * np.spacing(np.abs(np.asarray(wscore))))
    assert got == base[0] and np.array_equal(np.asarray(score), np.asarray(base[1])) and list(st) == list(base[2])


def _fast_plan(T, B, V, W, occ2):
    """The library's own plan (ops.beam_plan; tests/test_beam_plan_host.py holds it to the rule) with beam_occ2 = occ2: (takes the fast kernel,
    lm_lds, trie_slots).  False = ctcn_beam_decode silently takes the generic kernel instead, so the occ2 cases assert the branch they are
    meant to cover with it."""
    from ctc_pytorch_amd import ops
    ops.set_option("beam_occ2", occ2)
    try:
        p = ops.beam_plan(T, B, V, W)
    finally:
        ops.set_option("beam_occ2", 0)
    return p["path"] == (1 if occ2 else 0), bool(p["lm_lds"]), p["trie_slots"]


_OCC2_ORACLE = {}

# name: (V, T, B, W, regime, alpha, nbest, {occ2: (lm_lds, trie_slots)} or None)
OCC2_CASES = {
    "cfg5_flat": (62, 800, 16, 20, "flat", 0.1, 1, {1: (True, 4096), 2: (False, 8192)}),   # ~10 000 labellings: past the small LDS trie
    "w52_lm_global": (62, 160, 8, 52, "peaky", 0.1, 1, {1: (False, 1024), 2: (False, 4096)}),  # occ2 = 1: the LM does not fit next to the trie
    "v3_w2": (3, 70, 14, 2, "flat", 0.0, 1, None),
    "v4_w5": (4, 70, 14, 5, "flat", 0.5, 1, None),
    "v8_w33": (8, 70, 14, 33, "flat", 0.3, 1, None),
    "v5_w52": (5, 70, 14, 52, "flat", 1.0, 1, None),
    "nbest": (62, 160, 12, 20, "peaky", 0.1, 3, None),
}


@pytest.mark.parametrize("occ2", [1, 2])
@pytest.mark.parametrize("case", sorted(OCC2_CASES))
def test_beam_occ2_variants_vs_c_oracle(dev, case, occ2):
    """Option beam_occ2 = 1 / 2: the fast beam search compiled for two workgroups per CU, LM table in LDS or in global memory, with a 4 096 /
    8 192-slot LDS trie (16 384 by default), so that it spills to the global node table far earlier.  Labellings and status equal the C
    restatement of BeamSearch.py, float64 scores within 4 ulp, and everything bit for bit equal to beam_occ2 = 0.  Cases: a cfg5-shaped flat
    batch (the trie overflows), W = 52 where occ2 = 1 leaves the LM in global memory, small alphabets with beams wider than V and 0 / 1 / T
    frame utterances (test_beam_fuzz_small_alphabets_vs_c_oracle's), an n-best output.  Every case must take the fast kernel (_fast_plan)."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    V, T, B, W, regime, alpha, nbest, expect = OCC2_CASES[case]
    ok, lm_lds, slots = _fast_plan(T, B, V, W, occ2)
    assert ok, case
    if expect is not None:
        assert (lm_lds, slots) == expect[occ2], (case, lm_lds, slots)
    rs = np.random.RandomState(1000 * V + W)
    lp = synth.make_logprobs(seed=V * 7 + W, T=T, B=B, V=V, regime=regime)
    if V == 62:
        i2c = synth.int2char(V)
        tab = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(V)])
        lens = list(rs.randint(T // 2, T + 1, size=B))
    else:
        tab = -3.0 * rs.random_sample((V + 1, V + 1))
        lens = list(rs.randint(T // 3, T + 1, size=B))
        lens[0], lens[1], lens[2] = 0, 1, T
    probs = torch.exp(torch.from_numpy(lp))
    if case not in _OCC2_ORACLE:                       # (the C oracle once per case, for both variants)
        _OCC2_ORACLE[case] = beam_ref.decode_ids_nbest(probs.numpy().transpose(1, 0, 2), lens, tab, alpha, W, nbest)
    want, wscore, wst = _OCC2_ORACLE[case]
    runs = {}
    for o in (0, occ2):
        ops.set_option("beam_occ2", o)
        try:
            runs[o] = ops.beam_decode_nbest(probs.to(dev), lens, tab, alpha, W, nbest, 0, input_is_prob=True)
        finally:
            ops.set_option("beam_occ2", 0)
    got, score, st = runs[occ2]
    assert list(st) == list(wst), case
    assert got == want, case
    score, wscore = np.asarray(score), np.asarray(wscore)
    assert np.all(np.abs(score - wscore) <= 4 * np.spacing(np.abs(wscore))), case
    assert got == runs[0][0] and np.array_equal(score, np.asarray(runs[0][1])) and list(st) == list(runs[0][2])


def test_beam_width_above_the_maximum_is_refused(dev):
    """W = 1 025 > BEAM_WMAX: CTCN_EUNSUPPORTED (-3) from the C ABI, a RuntimeError naming the limit from the wrapper; nothing is launched."""
    from ctc_pytorch_amd import _lib, ops
    V, T, B = 62, 20, 2
    lp = torch.from_numpy(synth.make_logprobs(seed=5, T=T, B=B, V=V, regime="peaky")).to(dev)
    tab = np.zeros((V + 1, V + 1))
    with pytest.raises(RuntimeError, match="beam width 1025"):
        ops.beam_decode(lp, [T, T], tab, 0.1, 1025)
    L = _lib.lib()
    lens = torch.tensor([T, T], dtype=torch.int32, device=dev)
    lm = torch.zeros((V + 1) * (V + 1), dtype=torch.float64, device=dev)
    ws = torch.empty(max(L.ctcn_beam_ws_bytes(T, B, V, 256), 1), dtype=torch.uint8, device=dev)
    oi, ol = torch.zeros((B, T), dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    sc, stt = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    rc = L.ctcn_beam_decode(ctypes.c_void_p(lp.data_ptr()), 0, ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(lm.data_ptr()), 0.1, 1025, 0,
                            ctypes.c_void_p(oi.data_ptr()), ctypes.c_void_p(ol.data_ptr()), ctypes.c_void_p(sc.data_ptr()), ctypes.c_void_p(stt.data_ptr()),
                            T, B, V, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert rc == -3


def test_beam_decoder_reference_defaults_golden(dev):
    """BeamDecoder(int2char, lm_path=...) with every other argument at the reference's default (ctcDecoder.py:170: beam_width = 200,
    lm_alpha = 0.01, blank 0, no space symbol) on the golden log-probs: the strings the reference's interpreter loop returned
    (oracle/gen_golden.py gen_wide_beam -> tests/golden/decoders_wide.json), plus W = 60 / 61 / 128 at alpha 0.1."""
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    meta = json.load(open(os.path.join(G, "decoders_wide.json")))
    z = load("decoders")
    i2c = synth.int2char(62)
    arpa = os.path.join(G, "lm_phone_bg.arpa")
    for regime in ("peaky", "flat"):
        lp = torch.from_numpy(z["lp_" + regime])
        bd = BeamDecoder(i2c, lm_path=arpa)
        assert bd.beam_width == 200 and bd._decoder.lm_alpha == 0.01
        assert bd.decode(lp, meta["lens"]) == meta["beam_%s_default" % regime], regime
        for key in sorted(k for k in meta if k.startswith("beam_%s_W" % regime)):
            W = int(key.split("_W")[1].split("_")[0])
            bd = BeamDecoder(i2c, beam_width=W, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.1)
            assert bd.decode(lp, meta["lens"]) == meta[key], key


@pytest.mark.parametrize("V,W,regime,alpha", [(3, 2, "flat", 0.0), (4, 5, "flat", 0.5), (4, 20, "flat", 0.1), (8, 33, "flat", 0.3), (8, 52, "peaky", 0.1),
                                                 (5, 52, "flat", 1.0), (30, 10, "flat", 0.1), (200, 10, "peaky", 0.1), (200, 16, "flat", 0.2), (62, 1, "flat", 0.1),
                                                 (200, 20, "peaky", 0.1), (200, 40, "flat", 0.2)])     # (4 000 / 8 000 candidates per frame: the generic kernel with 1 024 threads)
def test_beam_fuzz_small_alphabets_vs_c_oracle(dev, V, W, regime, alpha):
    """Round 4 moved the prefix trie to a wave of its own: wave 0 recognises "this labelling's parent was created in this very frame" from
    (grandparent id, parent's last class) keys instead of node ids.  Small alphabets are what stresses that logic -- labellings leave the beam
    and come back, parents are re-created next to their children, nearly every slot merges -- so: V = 3 .. 8 with beams wider than the
    alphabet, one and two log-add passes (W <= 32 / > 32), the widest beam of the fast kernel (52), a 200-class alphabet (cfg4's), W = 1,
    zero-length and one-frame utterances, random LM tables.  Labellings and status equal the C restatement, float64 scores to the last places."""
    from ctc_pytorch_amd import ops
    T, B = 70, 14
    rs = np.random.RandomState(1000 * V + W)
    lp = synth.make_logprobs(seed=V * 7 + W, T=T, B=B, V=V, regime=regime)
    lens = list(rs.randint(T // 3, T + 1, size=B))
    lens[0], lens[1], lens[2] = 0, 1, T
    tab = -3.0 * rs.random_sample((V + 1, V + 1))
    probs = torch.exp(torch.from_numpy(lp))
    want, wscore, wst = beam_ref.decode_ids(probs.numpy().transpose(1, 0, 2), lens, tab, alpha, W)
    for fast in (1, 0):                  # (0: the generic kernel, whose selection -- pruning bound + rank count since round 5 -- these batches stress as well)
        ops.set_option("beam_fast", fast)
        try:
            got, score, st = ops.beam_decode(probs.to(dev), lens, tab, alpha, W, 0, input_is_prob=True)
        finally:
            ops.set_option("beam_fast", 1)
        assert list(st) == list(wst), fast
        assert got == [list(map(int, s_)) for s_ in want], fast
        # float64 scores: the device's exp / log (ocml) and glibc's differ in the last place on some arguments -- 0-2 ulp of the final score on
        # these batches, the same with the round-3 kernel (tools/beam_fuzz_ab.py runs both: bit-equal to each other); the golden sets are bit-equal
        score, wscore = np.asarray(score), np.asarray(wscore)
        assert np.all(np.abs(score - wscore) <= 4 * np.spacing(np.abs(wscore))), fast


@pytest.mark.parametrize("kind,V,W,alpha", [("uniform", 62, 20, 0.0), ("uniform", 62, 20, 0.1), ("uniform", 16, 52, 0.0), ("quantised", 62, 20, 0.0),
                                             ("quantised", 30, 40, 0.3), ("uniform", 62, 200, 0.0), ("quantised", 40, 100, 0.3), ("uniform", 8, 256, 0.1)])
def test_beam_exact_ties_vs_c_oracle(dev, kind, V, W, alpha):
    """Collisions, as this domain has them: EXACT ties of prTotal.  Uniform posteriors (every class 1 / V) make all extensions of a slot --
    and, from the second frame on, of all slots -- tie to the last bit; posteriors quantised to powers of two make most of them tie.  The
    reference ranks with a stable descending sort (BeamSearch.py:29-33), so ties resolve by insertion order, which the kernel restates as
    (prTotal desc, candidate index asc); hundreds of candidates then sit AT the pruning bound: more than the 256 survivors the rank count
    holds, i.e. the block-wide arg-max rounds that no random batch reaches (and, below 64, wave 2's per-survivor stay totals with tied keys).
    Labellings and status equal the C restatement; scores to the last places."""
    from ctc_pytorch_amd import ops
    T, B = 14, 6
    rs = np.random.RandomState(5 * V + W)
    if kind == "uniform":
        probs = np.full((T, B, V), 1.0 / V, dtype=np.float32)
    else:
        e = rs.randint(1, 4, size=(T, B, V))                 # 1/2, 1/4, 1/8 (not normalised: the search takes the probabilities as they are)
        probs = (0.5 ** e).astype(np.float32)
    lens = [T, T - 1, 1, 0, T // 2, T]
    tab = np.zeros((V + 1, V + 1)) if alpha == 0.0 else -np.round(3.0 * rs.random_sample((V + 1, V + 1)), 0)   # (integer LM scores: ties survive them)
    want, wscore, wst = beam_ref.decode_ids(probs.transpose(1, 0, 2), lens, tab, alpha, W)
    for fast in (1, 0):
        ops.set_option("beam_fast", fast)
        try:
            got, score, st = ops.beam_decode(torch.from_numpy(probs).to(dev), lens, tab, alpha, W, 0, input_is_prob=True)
        finally:
            ops.set_option("beam_fast", 1)
        assert list(st) == list(wst), fast
        assert got == [list(map(int, s_)) for s_ in want], fast
        score, wscore = np.asarray(score), np.asarray(wscore)
        assert np.all(np.abs(score - wscore) <= 4 * np.spacing(np.abs(wscore))), fast


@pytest.mark.parametrize("fast", [1, 0])
def test_beam_nbest_golden_and_oracle(dev, fast):
    """ctcn_beam_decode_nbest (the optional n-best output): the labellings equal the reference's whole final `last.sort()`
    (decoders_nbest.json, captured from the reference by oracle/gen_golden.py), ids and float64 scores equal the C oracle's on random
    batches for nbest = 1, 3 and W (the final beam can hold fewer than nbest entries), entry 0 equals ctcn_beam_decode; both kernels."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    z = load("decoders")
    meta = json.load(open(os.path.join(G, "decoders.json")))
    nb = json.load(open(os.path.join(G, "decoders_nbest.json")))
    V = 62
    i2c = synth.int2char(V)
    arpa = os.path.join(G, "lm_phone_bg.arpa")
    tab = LanguageModel(arpa).table([i2c[i] for i in range(V)])
    ops.set_option("beam_fast", fast)
    try:
        for key, rec in nb.items():
            _, regime, w, a = key.split("_")
            W, alpha = int(w[1:]), float(a[1:])
            N = min(W, 5)
            lpt = torch.from_numpy(z["lp_" + regime])
            ids, score, st = ops.beam_decode_nbest(torch.exp(lpt).to(dev), meta["lens"], tab, alpha, W, N, 0, input_is_prob=True)
            assert not st.any() and ids == rec["labellings"], key
            bd = BeamDecoder(i2c, beam_width=W, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=alpha)
            strings, sc2 = bd._decoder.decode_nbest(torch.exp(lpt).transpose(0, 1), meta["lens"], N)
            assert [u[0] for u in strings] == rec["best_string"] and np.array_equal(sc2, score)
        T, B = 160, 12
        for regime, W in (("peaky", 20), ("flat", 8), ("peaky", 3)):
            lp = synth.make_logprobs(seed=101 + W, T=T, B=B, V=V, regime=regime)
            lens = list(np.random.RandomState(5).randint(T // 2, T + 1, size=B))
            probs = torch.exp(torch.from_numpy(lp))
            one, s1, st1 = ops.beam_decode(probs.to(dev), lens, tab, 0.1, W, 0, input_is_prob=True)
            for N in (1, 3, W):
                N = min(N, W)
                want, wscore, wst = beam_ref.decode_ids_nbest(probs.numpy().transpose(1, 0, 2), lens, tab, 0.1, W, N)
                got, score, st = ops.beam_decode_nbest(probs.to(dev), lens, tab, 0.1, W, N, 0, input_is_prob=True)
                assert list(st) == list(wst) and got == want, (regime, W, N)
                assert np.allclose(score, wscore, rtol=1e-12, atol=1e-12)
                assert [u[0] for u in got] == one and np.array_equal(score[:, 0], s1)
        with pytest.raises(Exception):
            ops.beam_decode_nbest(probs.to(dev), lens, tab, 0.1, 3, 4, 0, input_is_prob=True)          # nbest > beam width
    finally:
        ops.set_option("beam_fast", 1)


def test_beam_error_paths(dev):
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    i2c = synth.int2char(62)
    bd = BeamDecoder(i2c, beam_width=5, lm_path=os.path.join(G, "lm_phone_bg.arpa"), lm_alpha=0.1)
    p = np.full((5, 1, 62), 1e-3, dtype=np.float32)
    p[:, :, 0] = 0.95
    with pytest.raises(IndexError):
        bd.decode(torch.log(torch.from_numpy(p)), [5])
    lp = np.full((5, 1, 62), np.log(1.0 / 62), dtype=np.float32)
    lp[2, 0, 7] = -200.0                                    # exp underflows to 0 -> math.log(0) in the reference
    with pytest.raises(ValueError):
        bd.decode(torch.from_numpy(lp), [5])
    with pytest.raises(TypeError):
        BeamDecoder(i2c, beam_width=5)                      # lm_path=None: open(None), as the reference


@pytest.mark.parametrize("workload,comm", [("cfg1", "0"), ("cfg2", "0"), ("cfg2", "1")])
def test_bench_under_torchrun_with_rccl_collectives(dev, workload, comm):
    """The driver's N>1 launch line, with one rank: torch.distributed.run -> process group on the nccl (= RCCL) backend ->
    parameter broadcast, flat-gradient all-reduce ordered behind the side stream, sync-BN all-reduces, max-over-ranks.
    CTCN_FORCE_COLLECTIVES=1 makes the single rank issue every collective (parallel.py).  cfg2: the layers are large enough for
    the weight-gradient side stream, so the per-layer slices are all-reduced DURING the backward pass (parallel.enable_overlap);
    comm = 1: through the C-ABI communicator (ctcn_comm_init / ctcn_comm_allreduce_sum_f32) instead of torch.distributed."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CTCN_FORCE_COLLECTIVES="1", CTCN_COMM=comm, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29517", os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", workload,
           "--sync-bn", "--full", "--no-cpu-baseline", "--no-decode", "--no-others", "--no-pmc"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 1 and res["steps"] == 2 and res["config"]["sync_bn"] is True
    assert res["value"] > 0 and np.isfinite(res["final_loss"])
    if workload == "cfg2":
        assert res["overlapped_allreduce_slices_last_step"] >= 2, res.get("overlapped_allreduce_slices_last_step")
    # RCCL's own account of the communicator (NCCL_DEBUG=INFO into a per-rank file, round 5) made it into the line
    assert res["comm"]["collectives_issued"] and len(res["per_rank_ms_per_step"]) == 1
    assert isinstance(res["comm"]["rccl_info"], list) and len(res["comm"]["rccl_info"]) > 0, res["comm"]


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_two_ranks_on_one_gpu_over_gloo(dev, scaling):
    """The N > 1 code path of bench.py end to end with two REAL ranks (the driver's launch form needs two GPUs; here both ranks share the one
    GPU and gloo carries the collectives, RCCL refusing two ranks per device): parameter broadcast, sharded seeds, the step-end all-reduce
    behind the side stream, barriers, max-over-ranks and the per-rank clocks of the line (round 5).  cfg1: both ranks' persistent grids
    (16 workgroups each) are co-resident.  Round 6: `--scaling strong` (the workload's batch is the GLOBAL batch, B / N utterances
    per rank) and the per-rank records of the RankMonitor (phase, status word, recurrence kernels) in `comm`."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641" if scaling == "weak" else "29643", WORLD_SIZE="2", LOCAL_RANK="0", CTCN_DIST_BACKEND="gloo",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1", CTCN_QUIET="1")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "cfg1", "--full", "--no-cpu-baseline",
           "--no-decode", "--no-others", "--no-pmc", "--scaling", scaling]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=280) for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[1][-2000:] for o in outs)
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and not [l for l in outs[1][0].splitlines() if l.startswith("{")]          # rank 0 alone prints the line
    res = json.loads(lines[0])
    per_rank_b = 8 if scaling == "weak" else 4
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 2 * per_rank_b and res["scaling"] == scaling
    assert len(res["per_rank_ms_per_step"]) == 2 and max(res["per_rank_ms_per_step"]) <= res["ms_per_step"] * 1.0001
    assert res["value"] > 0 and np.isfinite(res["final_loss"]) and res["comm"]["collectives_issued"] and res["comm"]["ranks"] == 2
    assert abs(res["value"] - 2 * per_rank_b * 300 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]      # whole-job frames / max-over-ranks time
    per_rank = res["comm"]["per_rank"]
    assert sorted(per_rank) == ["0", "1"] and res["comm"]["dp_safe"] is False
    for r in ("0", "1"):
        assert per_rank[r]["done"]["status"] == 0 and "step" not in "".join(per_rank[r]["done"]["kernels"]), per_rank[r]
        assert per_rank[r]["progress"]["phase"] == "timed"


def test_bench_rank_failure_yields_a_line_with_the_diagnosis(dev):
    """VERDICT r5 next 5, on the real bench.py: two ranks over gloo on the one GPU, rank 1 raises at step 3 of its prewarm loop
    (CTCN_BENCH_FAIL_RANK / _STEP) while rank 0 waits in that step's all-reduce.  Rank 0's JSON line must arrive within 150 s with `error`,
    every rank's last phase and the failing rank's message; both processes end with code 3.  CTCN_DP_SAFE=1 rides along: the line says so."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29645", WORLD_SIZE="2", LOCAL_RANK="0", CTCN_DIST_BACKEND="gloo", CTCN_DP_SAFE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1", CTCN_QUIET="1", CTCN_BENCH_FAIL_RANK="1", CTCN_BENCH_FAIL_STEP="3")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "cfg1", "--no-cpu-baseline",
           "--no-decode", "--no-others", "--no-pmc"]
    t0 = time.time()
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=150) for p in procs]
    assert time.time() - t0 < 150
    assert [p.returncode for p in procs] == [3, 3], "\n".join(o[1][-1500:] for o in outs)
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1, outs[0]
    res = json.loads(lines[0])
    assert res["value"] is None and "rank 1 failed" in res["error"] and "injected failure" in res["error"] and res["comm"]["dp_safe"] is True
    assert "injected failure" in res["ranks"]["1"]["failed"]["error"] and res["ranks"]["0"]["progress"]["phase"] == "prewarm"


@pytest.mark.parametrize("workload,steps", [("cfg2", 60), ("cfg4", 12)])
def test_persistent_recurrences_survive_foreign_resident_kernels(dev, workload, steps):
    """VERDICT r2 #1b / DESIGN section 6 (co-residency contract with RCCL): squatter kernels -- up to 12 workgroups per XCD parked for up
    to 4 ms on a third stream, what an RCCL kernel waiting for a slow peer looks like -- are launched at random points of training steps at
    precision 1 with the side stream, the pipelined projection and the gradient-slice hook on.  No hand-off may time out and the loss
    trajectory must equal the undisturbed run bit for bit.  cfg4 (H = 512, B = 64): the recurrence takes EVERY CU of all 8 XCDs, so a
    squatter that got there first delays whole launches."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import squat_stress
    trace = bool(os.environ.get("CTCN_TRAJ_LOG"))            # (per-step device-side checksums of activations / gradients / parameters into the log)
    base = squat_stress.run(workload, steps, squat=False, dev=dev, trace=trace)
    hit = squat_stress.run(workload, steps, squat=True, seed=3, dev=dev, trace=trace)
    print("undisturbed losses of %s: %r" % (workload, base["losses"][:7]))
    assert hit["squats"] >= steps // 2
    assert np.isfinite(hit["losses"]).all()
    if hit["losses"] != base["losses"]:          # say whether the undisturbed run itself repeats (then it is the squatters) or not (then it is not)
        again = squat_stress.run(workload, steps, squat=False, dev=dev, trace=trace)
        where = [(i, a, b) for i, (a, b) in enumerate(zip(hit["losses"], base["losses"])) if a != b][:5]
        assert False, ("disturbed != undisturbed at (step, disturbed, undisturbed) %r; a second undisturbed run is %s the first"
                       % (where, "EQUAL to" if again["losses"] == base["losses"] else "DIFFERENT from"))
    assert hit["kernels"][0] in ("rnn_fwd_tagged", "rnn_fwd_persist") and hit["kernels"][1] in ("rnn_bwd_scatter2", "rnn_bwd_scatter", "rnn_bwd_persist"), hit["kernels"]


def _spawn_ranks(args, world, port, extra_env=None, timeout=600):
    """`world` ranks on the ONE GPU of the box (LOCAL_RANK 0 for all; gloo carries the collectives, RCCL refuses two ranks per
    device).  The persistent recurrences need their whole grid co-resident, which two processes sharing the chip cannot promise
    each other: these runs use the one-launch-per-timestep kernels (same arithmetic, same summation order)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), LOCAL_RANK="0", CTCN_DIST_BACKEND="gloo",
               CTCN_RNN_PERSISTENT="0", CTCN_PRECISION="0", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1", CTCN_QUIET="1")
    env.update(extra_env or {})
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "dp_worker.py")] + args, env=dict(env, RANK=str(r)), cwd=root,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=timeout)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)


def test_data_parallel_two_ranks_equal_single_process(dev, tmp_path):
    """SURVEY 8a last gate / 8e: one global minibatch of 7 ragged utterances, (a) single process, (b) two ranks holding
    shards of 4 + 3 utterances padded to the GLOBAL T_max, loss = sum_shard nll / B_global, synchronised BatchNorm (1d over
    (T*B) rows, and 2d in the CNN variant) and one SUM all-reduce of the flat gradient: loss <= 1e-5 rel, gradient equal up
    to summation order, per-shard log-probs and BatchNorm running statistics equal."""
    out = str(tmp_path / "equiv.json")
    _spawn_ranks(["equiv", out], 2, 29631)
    res = json.load(open(out))
    for kind in ("rnn", "cnn"):
        r = res[kind]
        assert r["loss_rel"] < 1e-5, r
        assert r["grad_rel_l2"] < 2e-6 and r["grad_norm"] > 0, r
        assert r["lp_shard_maxabs"] < 2e-5 and r["running_stats_maxabs"] < 1e-6, r


def test_data_parallel_two_ranks_on_the_benchmarked_kernels(dev, tmp_path):
    """ The same equivalence on the kernels bench.py times: PERSISTENT recurrences (rnn_fwd_tagged / rnn_bwd_scatter)
    and bf16x3 GEMMs (precision 1), two ranks on the one GPU at H = 128, where both ranks' grids (2 directions x 1 batch tile x 8 slices
    = 16 workgroups each) are co-resident.  The reference is the single process at the same precision, so the gates are those of the f32
    run: the shards change the batch-tile composition and the order of the BatchNorm / gradient sums, not the per-row arithmetic."""
    out = str(tmp_path / "equiv_p.json")
    _spawn_ranks(["equiv", out], 2, 29639, extra_env={"CTCN_RNN_PERSISTENT": "1", "CTCN_PRECISION": "1", "CTCN_TEST_H": "128", "CTCN_TEST_PRECISION": "1"},
                 timeout=300)
    res = json.load(open(out))
    for kind in ("rnn", "cnn"):
        r = res[kind]
        assert r["precision"] == 1 and r["H"] == 128
        assert r["kernels"][0] in ("rnn_fwd_tagged", "rnn_fwd_persist") and r["kernels"][1] in ("rnn_bwd_scatter", "rnn_bwd_scatter2", "rnn_bwd_persist"), r
        assert r["loss_rel"] < 1e-5, r
        assert r["grad_rel_l2"] < 2e-5 and r["grad_norm"] > 0, r
        assert r["lp_shard_maxabs"] < 5e-5 and r["running_stats_maxabs"] < 1e-5, r


def test_data_parallel_overlap_is_rank_invariant(dev, tmp_path):
    """the early all-reduce of a recurrent layer's gradient slice is a collective, so every rank must decide alike.
    even = 16 + 16 utterances: both ranks reduce the top layer's slice early; uneven = 17 + 16 with the side-stream threshold between the
    two shard sizes (rank 0 alone would have issued the collective): nobody reduces early.  Both equal the single-process gradient."""
    out = str(tmp_path / "overlap.json")
    _spawn_ranks(["overlap", out], 2, 29637, timeout=300)
    res = json.load(open(out))
    assert res["even"]["early_slices_all_ranks"] == 2 * res["even"]["early_slices_rank0"] and res["even"]["early_slices_rank0"] >= 1, res
    assert res["uneven"]["early_slices_all_ranks"] == 0, res
    for k in ("even", "uneven"):
        assert res[k]["loss_rel"] < 1e-5 and res[k]["grad_rel_l2"] < 2e-6, res


def test_train_driver_data_parallel_matches_single_process(dev, tmp_path):
    """steps/train_ctc.main under WORLD_SIZE=2 (global minibatches sharded by parallel.ShardedBatches, global padding,
    global_batch scaling, sync BatchNorm, all-reduced statistics, rank-0 checkpoint) follows the 1-process run of the same
    YAML: same per-epoch train / dev losses and dev accuracy, same final parameters on both ranks."""
    from ctc_pytorch_amd.utils.data_loader import write_kaldi_ark
    rs = np.random.RandomState(11)
    phones = ["p%d" % i for i in range(8)]
    proto = rs.standard_normal((len(phones), 40)).astype(np.float32) * 2.0
    mats, labs = {}, {}
    for u in range(21):                                   # 21 utterances, batch 8: the last global batch has 5 (shards 3 + 2)
        seq = [int(k) for k in rs.randint(0, len(phones), size=int(rs.randint(4, 8)))]
        frames = [proto[k] + 0.3 * rs.standard_normal(40) for k in seq for _ in range(int(rs.randint(5, 9)))]
        mats["utt%02d" % u] = np.asarray(frames, dtype=np.float32)
        labs["utt%02d" % u] = " ".join(phones[k] for k in seq)
    d = str(tmp_path)
    write_kaldi_ark(d + "/feats.ark", d + "/feats.scp", mats)
    open(d + "/text", "w").write("".join("%s %s\n" % kv for kv in labs.items()))
    open(d + "/vocab", "w").write("".join("%d %s\n" % (i, ph) for i, ph in enumerate(phones)))
    _spawn_ranks(["main", d, d + "/w1"], 1, 29633)
    _spawn_ranks(["main", d, d + "/w2"], 2, 29635)
    one = json.load(open(d + "/w1.rank0"))
    two = [json.load(open(d + "/w2.rank%d" % r)) for r in range(2)]
    assert one["ckpt"] and two[0]["ckpt"] and not two[1]["ckpt"]              # rank 0 writes the package
    assert two[0]["hist"] == two[1]["hist"] and two[0]["param_sum"] == two[1]["param_sum"]
    for key in ("loss", "dev_loss"):
        assert np.allclose(two[0]["hist"][key], one["hist"][key], rtol=2e-4), (key, two[0]["hist"][key], one["hist"][key])
    assert np.allclose(two[0]["hist"]["dev_acc"], one["hist"]["dev_acc"], atol=0.02)
    assert abs(two[0]["param_norm"] - one["param_norm"]) / one["param_norm"] < 1e-4
    assert two[1]["lines"] == 0 and two[0]["lines"] > 0                       # one log stream
