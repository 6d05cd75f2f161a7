"""Operand alignment contract (DESIGN, "Operand alignment contract"): every ops.* function takes a contiguous float32 tensor at any
`data_ptr() % 16` and gives the aligned result.  The other GPU tests hand the kernels freshly allocated (256-byte aligned) tensors, so
the scalar side of every alignment gate -- vecA / vecB, the transposing split's vec, the inline A split, the TN tile, the split-K reduce, the
f32x4 reserve traffic of the recurrences -- has no other test.

Every operand here is placed at element offset k in {0, 1, 2, 3} of a larger buffer (`place`): 64 guard floats and more on each side, NaN
around an input, a fixed bit pattern around an output, which must be bit-unchanged after the call.  References and gates are those of the
aligned tests in test_gpu_kernels.py, named at each use; no tolerance is invented here."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as tnn

from oracle import np_ref as R
from oracle import torch_cpu
from ctc_pytorch_amd.testing import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))         # packed_ref, test_ctc_align_host

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats (256 bytes: the offset alone decides data_ptr() % 16)
PATTERN = 0x5A5AA5A5             # a finite float32 (1.5e16): also visible in a result that read it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f32_strict_unless_stated():
    from ctc_pytorch_amd import ops
    ops.set_precision(0)
    yield
    ops.set_precision(ops.DEFAULT_PRECISION)


class Placed(object):
    """A tensor of `shape` at element offset k of a guarded buffer.  value given: an input (NaN guards); None: an output (pattern guards,
    pattern payload unless `zero`)."""

    def __init__(self, dev, shape, k, value=None, zero=False):
        n = int(np.prod(shape))
        self.k, self.n = k, n
        self.buf = torch.empty(GUARD + 4 + n + GUARD + 4, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        if value is None:
            self.buf.view(torch.int32).fill_(PATTERN)
        else:
            self.buf.fill_(float("nan"))
        self.t = self.buf[GUARD + k:GUARD + k + n].view(shape)
        if value is not None:
            self.t.copy_(value.to(dev) if torch.is_tensor(value) else torch.from_numpy(np.ascontiguousarray(value)).to(dev))
        elif zero:
            self.t.zero_()
        assert self.t.data_ptr() % 16 == 4 * k and self.t.is_contiguous()

    def guards_intact(self):
        b = self.buf.view(torch.int32)
        lo, hi = b[:GUARD + self.k], b[GUARD + self.k + self.n:]
        return bool((lo == PATTERN).all()) and bool((hi == PATTERN).all())


def place(dev, value, k):
    return Placed(dev, tuple(value.shape), k, value=value)


def maxabs(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0


def rel_l2(a, b):
    a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# one operand at a time at offsets 1 and 2, then all of them at 1, 2 and 3
def offset_cases(names):
    cases = [{}]
    for n in names:
        cases += [{n: 1}, {n: 2}]
    return cases + [dict((n, k) for n in names) for k in (1, 2, 3)]


# ---------------------------------------------------------------------------------------------------------
# ops.gemm: reference and tolerance of test_gpu_kernels.test_gemm (float64 product; (2e-6 | 4e-5) * |A|max |B|max sqrt(K) * 4 + 1e-6)
# ---------------------------------------------------------------------------------------------------------
_ALL_T = [(0, 0), (0, 1), (1, 0), (1, 1)]
GEMM_CASES = ([(33, 17, 5, ta, tb, prec) for prec in (0, 1) for ta, tb in _ALL_T] +
              [(130, 68, 72, ta, tb, prec) for prec in (0, 1) for ta, tb in _ALL_T] +       # K >= 64: the plane path at precision 1; lda % 4 == 0
              [(200, 64, 1100, ta, tb, prec) for prec in (0, 1) for ta, tb in _ALL_T] +     # split-K and its vectorised reduce (N % 4 == 0)
              [(128, 32, 1024, 1, 0, 1)] +                                                   # TN tile when A and B are aligned
              [(8192, 768, 64, 0, tb, 1) for tb in (0, 1)])                                  # 256-row tiles: inline A split / plane split


@pytest.mark.parametrize("M,N,K,ta,tb,prec", GEMM_CASES)
def test_gemm_misaligned_operands(dev, M, N, K, ta, tb, prec):
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    rs = np.random.RandomState(M * 7 + N * 3 + K + ta * 2 + tb)
    A = rs.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    Bm = rs.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    C0 = rs.standard_normal((M, N)).astype(np.float32)
    want = (A.T if ta else A).astype(np.float64) @ (Bm.T if tb else Bm).astype(np.float64)
    scale = np.abs(A).max() * np.abs(Bm).max() * np.sqrt(K)
    tol = (2e-6 if prec == 0 else 4e-5) * scale * 4 + 1e-6
    big = M >= 8192
    for beta in (0.0, 1.0):
        ref = want + beta * C0
        aligned = None
        for mis in (offset_cases("ABC")[:7] + offset_cases("ABC")[-1:] if big else offset_cases("ABC")):
            a, b = place(dev, A, mis.get("A", 0)), place(dev, Bm, mis.get("B", 0))
            c = Placed(dev, (M, N), mis.get("C", 0))
            c.t.copy_(torch.from_numpy(C0).to(dev))
            ops.gemm(ta, tb, M, N, K, a.t, A.shape[1], b.t, Bm.shape[1], c.t, N, beta=beta)
            got = c.t.cpu().numpy()
            what = (ta, tb, M, N, K, prec, beta, mis)
            assert c.guards_intact(), ("wrote outside C", what)
            assert not np.isnan(got).any(), ("NaN: a guard was read", what)
            err = np.max(np.abs(got - ref))
            assert err < tol, (what, err, tol)
            if not mis:
                aligned = got
            elif set(mis) == {"C"} and K >= 1024:
                # A and B as in the aligned call: the same split-K partials, and splitk_reduce_kernel's 16-byte form does "the same additions
                # in the same order, bit-identical to the scalar form" (gemm.hip)
                assert np.array_equal(got, aligned), ("split-K reduce: scalar form differs from the 16-byte form", what)
    ops.set_precision(0)


# ---------------------------------------------------------------------------------------------------------
# ops.rnn_layer: torch.nn.{LSTM,GRU,RNN}(bias=False) on the CPU, at the gates of test_gpu_kernels.test_rnn_layer_vs_torch_cpu (precision 0:
# y max-abs 2e-5, gradients rel-L2 1e-4) and test_rnn_layer_bf16x3_vs_torch_cpu (precision 1: 1e-4 and 5e-4)
# ---------------------------------------------------------------------------------------------------------
_RNN_NAMES = ["weight_ih_l0", "weight_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse"]
_RNN_REF = {}


def _rnn_reference(kind, T, B, I, H, bi):
    key = (kind, T, B, I, H, bi)
    if key not in _RNN_REF:
        cls = {"lstm": tnn.LSTM, "gru": tnn.GRU, "tanh": tnn.RNN}[kind]
        torch.manual_seed(T * 100 + B)
        ref = cls(I, H, bidirectional=bi, bias=False)
        x, dy = torch.randn(T, B, I), torch.randn(T, B, (2 if bi else 1) * H)
        xr = x.clone().requires_grad_(True)
        yr, _ = ref(xr)
        yr.backward(dy)
        names = _RNN_NAMES if bi else _RNN_NAMES[:2]
        _RNN_REF[key] = dict(x=x, dy=dy, y=yr.detach(), dx=xr.grad.detach(), w=[getattr(ref, n).detach() for n in names],
                             dw=[getattr(ref, n).grad.detach() for n in names], names=names)
    return _RNN_REF[key]


def _run_rnn(dev, kind, ref, mis, drop=None):
    """The layer with x / the weights / dy at the offsets of `mis` (keys x, w0..w3, dy); with key g the weight gradients go, as with
    optim.FlatAdam, to `_ctcn_grad` views (beta = 1, the into_flat path) cut from buffers at that offset.
    drop: None, "fused" (the layer's own dropout) or "separate" (ops.dropout behind the layer), p = 0.2 at a fixed Philox position."""
    from ctc_pytorch_amd import ops
    nw = len(ref["w"])
    x = place(dev, ref["x"], mis.get("x", 0)).t.requires_grad_(True)
    w = [place(dev, ref["w"][i], mis.get("w%d" % i, 0)).t.requires_grad_(True) for i in range(nw)] + [None] * (4 - nw)
    dst = None
    if "g" in mis:
        dst = [Placed(dev, tuple(ref["w"][i].shape), mis["g"], zero=True) for i in range(nw)]
        for p, d in zip(w, dst):
            p._ctcn_grad = d.t
    dy = place(dev, ref["dy"], mis.get("dy", 0)).t
    if drop is not None:
        ops._drop_counter[0] = 1000
    if drop == "fused":
        y = ops.rnn_layer(x, w[0], w[1], w[2], w[3], kind, training=True, drop_p=0.2)
    else:
        y = ops.rnn_layer(x, w[0], w[1], w[2], w[3], kind)
        if drop == "separate":
            y = ops.dropout(y, 0.2, True)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    ops.check_health()
    if dst is not None:
        assert all(p.grad is None for p in w[:nw]), "into_flat: the gradients go to the views"
        assert all(d.guards_intact() for d in dst), ("wrote outside a weight-gradient view", mis)
        dws = [d.t.clone() for d in dst]
    else:
        dws = [p.grad for p in w[:nw]]
    return y.detach(), x.grad, dws


_RNN_OPERANDS = ["x", "w0", "w1", "w2", "w3", "dy", "g"]
RNN_SHAPES = [("lstm", 5, 3, 10, 16, True), ("lstm", 5, 3, 10, 16, False), ("gru", 4, 17, 12, 32, True), ("gru", 4, 17, 12, 32, False),
              ("tanh", 5, 3, 4, 16, False), ("tanh", 5, 3, 4, 16, True)]


def _check_rnn(got, ref, prec, what):
    y, dx, dws = got
    tol_y, tol_g = (2e-5, 1e-4) if prec == 0 else (1e-4, 5e-4)
    for t in [y, dx] + dws:
        assert not torch.isnan(t).any(), ("NaN: a guard was read", what)
    assert maxabs(y, ref["y"]) < tol_y, (what, maxabs(y, ref["y"]))
    assert rel_l2(dx, ref["dx"]) < tol_g, (what, "dx", rel_l2(dx, ref["dx"]))
    for n, g, wg in zip(ref["names"], dws, ref["dw"]):
        assert rel_l2(g, wg) < tol_g, (what, n, rel_l2(g, wg))


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("kind,T,B,I,H,bi", RNN_SHAPES)
def test_rnn_layer_misaligned_operands(dev, kind, T, B, I, H, bi, prec):
    """A misaligned W_hh (the operand ctcn_rnn_fwd refuses) is copied by ops.rnn_layer; everything else reaches the kernels as it is."""
    from ctc_pytorch_amd import ops
    ref = _rnn_reference(kind, T, B, I, H, bi)
    names = [n for n in _RNN_OPERANDS if not (n in ("w2", "w3") and not bi)]
    ops.set_precision(prec)
    try:
        for mis in offset_cases(names):
            _check_rnn(_run_rnn(dev, kind, ref, mis), ref, prec, (kind, T, B, I, H, bi, prec, mis))
    finally:
        ops.set_precision(0)


@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("prec", [0, 1])
def test_rnn_layer_misaligned_operands_persistent_kernels(dev, prec, persistent):
    """(lstm, T 8, B 32, I 40, H 320, bidirectional): the shape of cfg2's layers, which the persistent kernels take -- checked -- and the same
    with one launch per timestep."""
    from ctc_pytorch_amd import ops
    kind, T, B, I, H, bi = "lstm", 8, 32, 40, 320, True
    ref = _rnn_reference(kind, T, B, I, H, bi)
    before = ops.get_option("rnn_persistent")
    ops.set_precision(prec)
    ops.set_rnn_persistent(persistent)
    try:
        for mis in offset_cases(_RNN_OPERANDS):
            _check_rnn(_run_rnn(dev, kind, ref, mis), ref, prec, (kind, prec, persistent, mis))
            fwd, bwd = ops.rnn_last_kernels()[:2]
            if persistent:
                assert fwd in ("rnn_fwd_tagged", "rnn_fwd_persist") and bwd in ("rnn_bwd_scatter2", "rnn_bwd_scatter", "rnn_bwd_persist"), (fwd, bwd, mis)
            else:
                assert (fwd, bwd) == ("rnn_fwd_step", "rnn_bwd_step"), (fwd, bwd, mis)
    finally:
        ops.set_rnn_persistent(before)
        ops.set_precision(0)


def test_rnn_bwd_item_gather_leaves_scatter2_when_dy_is_misaligned(dev):
    """bwd_choose_formulation (rnn.hip) takes rnn_bwd_scatter2 -- 16-byte LDS DMA on dy -- only when dy is on 16 bytes.  At H = 320 the default
    never takes it, so option bwd_item_gather = 2 forces it, as test_gpu_kernels.test_rnn_bwd_item_gather_equals_scatter does: scatter2 with an
    aligned dy, another kernel with dy at offset 1, 2 or 3, both at the precision-1 gates of test_rnn_layer_bf16x3_vs_torch_cpu."""
    from ctc_pytorch_amd import ops
    kind, T, B, I, H, bi = "lstm", 8, 32, 40, 320, True
    ref = _rnn_reference(kind, T, B, I, H, bi)
    before = ops.get_option("bwd_item_gather")
    ops.set_precision(1)
    ops.set_option("bwd_item_gather", 2)
    try:
        for k in (0, 1, 2, 3):
            mis = {"dy": k} if k else {}
            _check_rnn(_run_rnn(dev, kind, ref, mis), ref, 1, ("item gather", mis))
            bwd = ops.rnn_last_kernels()[1]
            if k == 0:
                assert bwd == "rnn_bwd_scatter2", bwd
            else:
                assert bwd in ("rnn_bwd_scatter", "rnn_bwd_persist"), (bwd, mis)
    finally:
        ops.set_option("bwd_item_gather", before)
        ops.set_precision(0)


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("kind,T,B,I,H,bi", [("lstm", 8, 32, 40, 320, True), ("gru", 4, 17, 12, 32, True)])
def test_rnn_layer_fused_dropout_misaligned_equals_layer_then_dropout(dev, kind, T, B, I, H, bi, prec):
    """As test_gpu_kernels.test_rnn_layer_with_fused_dropout_equals_layer_then_dropout: output and every gradient of the layer's own dropout
    are bit-identical to the layer followed by ops.dropout at the same Philox position -- here with misaligned operands."""
    from ctc_pytorch_amd import ops
    ref = _rnn_reference(kind, T, B, I, H, bi)
    ops.set_precision(prec)
    try:
        for mis in ({}, {"x": 1}, {"dy": 2}, {"g": 1}, dict((n, 1) for n in _RNN_OPERANDS), dict((n, 2) for n in _RNN_OPERANDS)):
            ys, dxs, dws = _run_rnn(dev, kind, ref, mis, drop="separate")
            yf, dxf, dwf = _run_rnn(dev, kind, ref, mis, drop="fused")
            assert 0.6 < float((ys != 0).float().mean()) < 0.95
            assert torch.equal(ys, yf) and torch.equal(dxs, dxf), mis
            assert all(torch.equal(a, b) for a, b in zip(dws, dwf)), mis
    finally:
        ops.set_precision(0)


def test_rnn_layer_misaligned_w_hh_is_not_refused(dev):
    """ctcn_rnn_fwd requires a 16-byte aligned W_hh; ops.rnn_layer meets that with an aligned temporary and returns the gradient in the shape
    of the caller's view."""
    from ctc_pytorch_amd import ops
    ref = _rnn_reference("lstm", 5, 3, 10, 16, False)
    for k in (1, 2, 3):
        y, dx, dws = _run_rnn(dev, "lstm", ref, {"w1": k})
        _check_rnn((y, dx, dws), ref, 0, ("w_hh", k))
        assert dws[1].shape == ref["w"][1].shape


# ---------------------------------------------------------------------------------------------------------
# BatchNorm (plain, length-aware, fused dropout).  ops allocates y and dx itself (always on 16 bytes), so through ops the operands that can be
# misaligned are x, gamma, beta, the running statistics, dy and the dgamma / dbeta views.  One misaligned pointer among x / y / gamma / beta /
# mean / rstd sends launch_bn_apply and launch_bn_dx (`io | ch`: the dense rows4 kernels; `io`: the length-aware V = 4 streams, stream_vec,
# load_valid / store_all) and the column sums (aligned16()) to their dword side.
#   plain:  oracle/np_ref.py in float64 at the gates of test_gpu_kernels.test_batchnorm_branch_matrix_vs_oracle (y, dx, eval 2e-5 scaled by
#           magnitude; dgamma / dbeta rel-L2 1e-5; running statistics 1e-5 scaled)
#   masked: the float64 restatement and gates of test_length_mask.test_masked_kernels_against_float64 (y, dx, eval 2e-5 scaled; running
#           statistics relative 2e-5; dgamma / dbeta 2e-5 scaled); x and dy hold NaN at every padded element
#   fused dropout: bit for bit the two passes it replaces, as test_gpu_kernels.test_bn_relu_dropout_fused_equals_two_passes
# and y, dx and the eval output bit for bit those of offset 0: bn_value / bn_dx_value are "ONE rounding sequence" on every path (norm.hip).
# ---------------------------------------------------------------------------------------------------------
BN_ALIGN_CASES = {   # outer, C, inner, lengths, frame
    "rows4_c8": (150, 8, 1, [50, 1, 20], 1),        # inner == 1, C % 4 == 0: the rows4 kernels while every pointer is on 16 bytes (three 64-row tiles)
    "rows_c5": (150, 5, 1, [50, 1, 20], 1),         # C = 5: the dword kernels whatever the pointers
    "nchw_vec": (3, 5, 240, [40, 1, 17], 6),        # inner % 4 == 0: 16-byte streams when aligned
    "nchw_scalar": (3, 4, 35, [5, 1, 3], 7),        # inner % 4 != 0
}
_BN_OPERANDS = ["x", "gamma", "beta", "rm", "rv", "dy", "g"]
_BN_DATA = {}


def _bn_data(case):
    if case not in _BN_DATA:
        outer, C, inner, lens, frame = BN_ALIGN_CASES[case]
        rs = np.random.RandomState(outer + 7 * C + inner)
        shape = (outer, C) if inner == 1 else (outer, C, inner)
        d = dict(geom=BN_ALIGN_CASES[case], shape=shape)
        d["x"] = (rs.standard_normal(shape) * 2.5 + rs.standard_normal((1, C) + (1,) * (len(shape) - 2))).astype(np.float32)
        d["gamma"] = (rs.random_sample(C) + 0.5).astype(np.float32)
        d["beta"] = (rs.standard_normal(C) * 0.3).astype(np.float32)
        d["dy"] = rs.standard_normal(shape).astype(np.float32)
        d["rm"] = (rs.standard_normal(C) * 0.1).astype(np.float32)
        d["rv"] = (rs.random_sample(C) + 0.5).astype(np.float32)
        ln = np.asarray(lens)
        if inner == 1:                        # the validity rule of include/ctcn.h: time-major rows / NCHW planes
            r = np.arange(outer)
            v = np.broadcast_to(((r // len(lens)) < ln[r % len(lens)])[:, None], shape)
        else:
            v = np.broadcast_to(((np.arange(inner)[None, :] // frame) < ln[:, None])[:, None, :], shape)
        d["valid"] = np.ascontiguousarray(v)
        _BN_DATA[case] = d
    return _BN_DATA[case]


def _nan_guards_intact(p):
    return bool(torch.isnan(p.buf[:GUARD + p.k]).all()) and bool(torch.isnan(p.buf[GUARD + p.k + p.n:]).all())


def _run_bn(dev, d, mis, relu, mode):
    """mode: "plain" | "masked" | "drop_fused" | "drop_two" -> [y, dx, dgamma, dbeta, running_mean, running_var, eval output]."""
    from ctc_pytorch_amd import ops
    outer, C, inner, lens, frame = d["geom"]
    hide = (lambda a: np.where(d["valid"], a, np.float32("nan")).astype(np.float32)) if mode == "masked" else (lambda a: a)
    x = place(dev, hide(d["x"]), mis.get("x", 0)).t.requires_grad_(True)
    g = place(dev, d["gamma"], mis.get("gamma", 0)).t.requires_grad_(True)
    b = place(dev, d["beta"], mis.get("beta", 0)).t.requires_grad_(True)
    rm, rv = place(dev, d["rm"], mis.get("rm", 0)), place(dev, d["rv"], mis.get("rv", 0))
    dy = place(dev, hide(d["dy"]), mis.get("dy", 0)).t
    dst = None
    if "g" in mis:                            # dgamma / dbeta accumulate (beta = 1) into views, as with optim.FlatAdam
        dst = [Placed(dev, (C,), mis["g"], zero=True) for _ in range(2)]
        g._ctcn_grad, b._ctcn_grad = dst[0].t, dst[1].t
    fr = frame if inner > 1 else None
    if mode == "masked":
        y = ops.batch_norm_masked(x, g, b, rm.t, rv.t, outer, C, inner, True, lens, fr, 0.1, 1e-5, relu)
    elif mode == "plain":
        y = ops.batch_norm(x, g, b, rm.t, rv.t, outer, C, inner, True, 0.1, 1e-5, relu)
    else:
        ops.set_fuse_bn_dropout(mode == "drop_fused")
        ops._drop_counter[0] = 1234
        try:
            y = ops.batch_norm(x, g, b, rm.t, rv.t, outer, C, inner, True, 0.1, 1e-5, relu, None, drop_p=0.3)
        finally:
            ops.set_fuse_bn_dropout(True)
    y.backward(dy)
    if mode == "masked":
        ye = ops.batch_norm_masked(x.detach(), g.detach(), b.detach(), rm.t, rv.t, outer, C, inner, False, lens, fr, 0.1, 1e-5, relu)
    else:
        ye = ops.batch_norm(x.detach(), g.detach(), b.detach(), rm.t, rv.t, outer, C, inner, False, 0.1, 1e-5, relu)
    torch.cuda.synchronize()
    assert _nan_guards_intact(rm) and _nan_guards_intact(rv), ("wrote outside a running statistic", mis)
    if dst is not None:
        assert g.grad is None and b.grad is None, "into_flat: the gradients go to the views"
        assert all(q.guards_intact() for q in dst), ("wrote outside dgamma / dbeta", mis)
        dg, db = dst[0].t, dst[1].t
    else:
        dg, db = g.grad, b.grad
    return [t.detach().cpu().clone() for t in (y, x.grad, dg, db, rm.t, rv.t, ye)]


def _check_bn_plain(got, d, relu, what):
    outer, C, inner = d["geom"][:3]
    y, dx, dg, db, rm, rv, ye = got
    to2 = lambda a: np.asarray(a, dtype=np.float64).reshape(outer, C, inner).transpose(0, 2, 1).reshape(-1, C)
    g64, b64 = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    x2, dy2 = to2(d["x"]), to2(d["dy"])
    y_ref, mean, var = R.bn_train_fwd(x2, g64, b64)
    mask = np.ones_like(y_ref)
    if relu:
        mask = (to2(y.numpy()) > 0).astype(np.float64)          # the kernel's own ReLU mask, which is the oracle's away from 0
        sure = np.abs(y_ref) > 1e-4
        assert np.array_equal(mask[sure], (y_ref[sure] > 0).astype(np.float64)), what
        y_ref = np.maximum(y_ref, 0.0)
    dx_ref, dg_ref, db_ref = R.bn_train_bwd(x2, g64, mean, var, dy2 * mask)
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    assert maxabs(to2(y.numpy()), y_ref) < 2e-5 * scale(y_ref), what
    assert maxabs(to2(dx.numpy()), dx_ref) < 2e-5 * scale(dx_ref), what
    assert rel_l2(dg, dg_ref) < 1e-5 and rel_l2(db, db_ref) < 1e-5, (what, rel_l2(dg, dg_ref), rel_l2(db, db_ref))
    rm_ref, rv_ref = R.bn_running_update(d["rm"].astype(np.float64), d["rv"].astype(np.float64), mean, var, x2.shape[0], 0.1)
    assert maxabs(rm, rm_ref) < 1e-5 * scale(rm_ref) and maxabs(rv, rv_ref) < 1e-5 * scale(rv_ref), what
    ye_ref = R.bn_eval_fwd(x2, g64, b64, rm.numpy().astype(np.float64), rv.numpy().astype(np.float64))
    if relu:
        ye_ref = np.maximum(ye_ref, 0.0)
    assert maxabs(to2(ye.numpy()), ye_ref) < 2e-5 * scale(ye_ref), what


def _check_bn_masked(got, d, relu, what):
    C = d["geom"][1]
    y, dx, dg, db, rm, rv, ye = (t.numpy() for t in got)
    v = d["valid"]
    ax = tuple(i for i in range(v.ndim) if i != 1)
    bc = lambda a: a.reshape((1, C) + (1,) * (v.ndim - 2))
    x64, dy64 = d["x"].astype(np.float64), d["dy"].astype(np.float64)
    gamma, beta = bc(d["gamma"].astype(np.float64)), bc(d["beta"].astype(np.float64))
    n = float(v.sum()) / C
    mean = np.where(v, x64, 0).sum(ax) / n
    var = np.where(v, (x64 - bc(mean)) ** 2, 0).sum(ax) / n
    rstd = 1.0 / np.sqrt(var + 1e-5)
    xh = (x64 - bc(mean)) * bc(rstd)
    y_ref = xh * gamma + beta
    keep = np.ones_like(v)
    if relu:
        keep = y > 0                                             # the kernel's own ReLU mask, which is the restatement's away from 0
        sure = v & (np.abs(y_ref) > 1e-4)
        assert np.array_equal(keep[sure], y_ref[sure] > 0), what
    y_ref = np.where(v, np.maximum(y_ref, 0) if relu else y_ref, 0)
    gg = np.where(v & keep, dy64, 0)
    s0, s1 = gg.sum(ax), np.where(v, gg * xh, 0).sum(ax)
    dx_ref = np.where(v, gamma * bc(rstd) * (gg - bc(s0) / n - xh * bc(s1) / n), 0)
    for a in (y, dx, ye):
        assert np.isfinite(a).all() and np.all(a[~v] == 0), ("a padded element was read or written", what)
    assert np.max(np.abs(y - y_ref)) < 2e-5, what
    assert np.max(np.abs(dx - dx_ref)) < 2e-5 * max(1.0, float(np.abs(dx_ref).max())), what
    rel = lambda a, r: float(np.max(np.abs(a.astype(np.float64) - r) / np.maximum(np.abs(r), 1e-3)))
    assert rel(rm, 0.9 * d["rm"] + 0.1 * mean) < 2e-5 and rel(rv, 0.9 * d["rv"] + 0.1 * var * n / (n - 1)) < 2e-5, what
    scale = max(1.0, float(np.abs(s1).max()), float(np.abs(s0).max()))
    assert np.max(np.abs(dg - s1)) < 2e-5 * scale and np.max(np.abs(db - s0)) < 2e-5 * scale, what
    ye_ref = (x64 - bc(rm.astype(np.float64))) / np.sqrt(bc(rv.astype(np.float64)) + 1e-5) * gamma + beta
    ye_ref = np.where(v, np.maximum(ye_ref, 0) if relu else ye_ref, 0)
    assert np.max(np.abs(ye - ye_ref)) < 2e-5 * max(1.0, float(np.abs(ye_ref).max())), what


@pytest.mark.parametrize("mode", ["plain", "masked"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", sorted(BN_ALIGN_CASES))
def test_batch_norm_misaligned_operands(dev, case, relu, mode):
    d = _bn_data(case)
    check = _check_bn_plain if mode == "plain" else _check_bn_masked
    base = None
    for mis in offset_cases(_BN_OPERANDS):
        got = _run_bn(dev, d, mis, relu, mode)
        what = (case, relu, mode, mis)
        assert all(not torch.isnan(t).any() for t in got), ("NaN: a guard or a padded element was read", what)
        check(got, d, relu, what)
        if base is None:
            base = got
        for i, name in ((0, "y"), (1, "dx"), (6, "eval")):
            assert torch.equal(got[i], base[i]), ("bn_value / bn_dx_value: not the bits of the aligned call", name, what)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", sorted(BN_ALIGN_CASES))
def test_batch_norm_fused_dropout_misaligned_equals_two_passes(dev, case, relu):
    d = _bn_data(case)
    base = None
    for mis in offset_cases(_BN_OPERANDS):
        fused, two = _run_bn(dev, d, mis, relu, "drop_fused"), _run_bn(dev, d, mis, relu, "drop_two")
        for a, c, name in zip(fused, two, ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var", "eval")):
            assert torch.equal(a, c), (name, case, relu, mis)
        if base is None:
            base = fused
        for i in (0, 1, 6):
            assert torch.equal(fused[i], base[i]), (i, case, relu, mis)


def test_mask_frames_misaligned(dev):
    """ops.mask_frames in its three layouts, forward and backward, exact (a select), as test_length_mask.test_mask_frames_autograd_and_layouts;
    x and dy hold NaN at the padded frames."""
    from ctc_pytorch_amd import ops
    lens = [5, 1, 3]
    rs = np.random.RandomState(4)
    for layout, shape, taxis, baxis in (("tbc", (5, 3, 8), 0, 1), ("tbc", (5, 3, 5), 0, 1), ("btf", (3, 5, 6), 1, 0), ("bctf", (3, 2, 5, 6), 2, 0),
                                        ("bctf", (3, 5, 5, 7), 2, 0)):
        vt, vb = [1] * len(shape), [1] * len(shape)
        vt[taxis], vb[baxis] = shape[taxis], shape[baxis]
        m = np.broadcast_to(np.arange(shape[taxis]).reshape(vt) < np.asarray(lens).reshape(vb), shape)
        x0 = np.where(m, rs.standard_normal(shape), np.nan).astype(np.float32)
        dy0 = np.where(m, rs.standard_normal(shape), np.nan).astype(np.float32)
        for mis in offset_cases(["x", "dy"]):
            x = place(dev, x0, mis.get("x", 0)).t.requires_grad_(True)
            y = ops.mask_frames(x, torch.tensor(lens), layout)
            y.backward(place(dev, dy0, mis.get("dy", 0)).t)
            assert np.array_equal(y.detach().cpu().numpy(), np.where(m, x0, 0).astype(np.float32)), (layout, shape, mis)
            assert np.array_equal(x.grad.cpu().numpy(), np.where(m, dy0, 0).astype(np.float32)), (layout, shape, mis)


# ---------------------------------------------------------------------------------------------------------
# ops.conv2d / ops.max_pool2d: oracle/np_ref.py in float64 at the gates of test_gpu_kernels.test_conv2d_vs_oracle (y 2e-6 |y|max sqrt(Ci kh kw),
# dx 2e-6 |dx|max sqrt(Co kh kw), dW / db rel-L2 2e-6), both kernel families; pooling bit-exact as test_maxpool2d_vs_oracle
# ---------------------------------------------------------------------------------------------------------
CONV_ALIGN_CASES = [(2, 32, 21, 20, 32, 3, 3, 2, 2, 1, 1),        # CONV_CASES[1]: the reference's second layer
                    (2, 3, 9, 11, 5, 3, 2, 1, 1, 0, 1),           # CONV_CASES[2]: ragged in both MFMA dimensions
                    (3, 3, 13, 20, 5, 3, 3, 1, 2, 1, 1)]          # 3 -> 5 channels, 3 x 3: the odd model's second layer (135 weights, 5 biases)
_CONV_REF = {}


def _conv_reference(case):
    if case not in _CONV_REF:
        B, Ci, Hi, Wi, Co, kh, kw, sh, sw, ph, pw = case
        rs = np.random.RandomState(sum(case))
        x = rs.standard_normal((B, Ci, Hi, Wi)).astype(np.float32)
        w = (rs.standard_normal((Co, Ci, kh, kw)) / np.sqrt(Ci * kh * kw)).astype(np.float32)
        b = rs.standard_normal(Co).astype(np.float32)
        y = R.conv2d_fwd(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), (sh, sw), (ph, pw))
        dy = rs.standard_normal(y.shape).astype(np.float32)
        dx, dw, db = R.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), (sh, sw), (ph, pw), dy.astype(np.float64))
        _CONV_REF[case] = dict(x=x, w=w, b=b, dy=dy, y=y, dx=dx, dw=dw, db=db)
    return _CONV_REF[case]


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("case", CONV_ALIGN_CASES)
def test_conv2d_misaligned_operands(dev, case, mfma):
    from ctc_pytorch_amd import ops
    B, Ci, Hi, Wi, Co, kh, kw, sh, sw, ph, pw = case
    r = _conv_reference(case)
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    before = ops.get_option("conv_mfma")
    ops.set_option("conv_mfma", mfma)
    try:
        for mis in offset_cases(["x", "w", "b", "dy", "g"]):
            x = place(dev, r["x"], mis.get("x", 0)).t.requires_grad_(True)
            w = place(dev, r["w"], mis.get("w", 0)).t.requires_grad_(True)
            b = place(dev, r["b"], mis.get("b", 0)).t.requires_grad_(True)
            dst = None
            if "g" in mis:
                dst = [Placed(dev, r["w"].shape, mis["g"], zero=True), Placed(dev, r["b"].shape, mis["g"], zero=True)]
                w._ctcn_grad, b._ctcn_grad = dst[0].t, dst[1].t
            y = ops.conv2d(x, w, b, (sh, sw), (ph, pw))
            y.backward(place(dev, r["dy"], mis.get("dy", 0)).t)
            torch.cuda.synchronize()
            if dst is not None:
                assert w.grad is None and b.grad is None and all(q.guards_intact() for q in dst), ("wrote outside dW / db", mis)
                dw, db = dst[0].t, dst[1].t
            else:
                dw, db = w.grad, b.grad
            for t in (y, x.grad, dw, db):
                assert not torch.isnan(t).any(), ("NaN: a guard was read", case, mfma, mis)
            assert maxabs(y, r["y"]) < 2e-6 * scale(r["y"]) * np.sqrt(Ci * kh * kw), (case, mfma, mis)
            assert maxabs(x.grad, r["dx"]) < 2e-6 * scale(r["dx"]) * np.sqrt(Co * kh * kw), (case, mfma, mis)
            assert rel_l2(dw, r["dw"]) < 2e-6 and rel_l2(db, r["db"]) < 2e-6, (case, mfma, mis, rel_l2(dw, r["dw"]), rel_l2(db, r["db"]))
    finally:
        ops.set_option("conv_mfma", before)


@pytest.mark.parametrize("shape,k", [((2, 3, 9, 8), (2, 2)), ((1, 2, 7, 5), (3, 1)), ((3, 5, 61, 10), (2, 1))])
def test_max_pool2d_misaligned(dev, shape, k):
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(sum(shape) + k[0])
    x0 = np.maximum(rs.standard_normal(shape), 0).astype(np.float32)          # ReLU output: many exact ties at 0
    y_ref, arg = R.maxpool2d_fwd(x0, *k)
    dy0 = rs.standard_normal(y_ref.shape).astype(np.float32)
    dx_ref = R.maxpool2d_bwd(dy0, arg, shape, *k)
    for mis in offset_cases(["x", "dy"]):
        x = place(dev, x0, mis.get("x", 0)).t.requires_grad_(True)
        y = ops.max_pool2d(x, k)
        y.backward(place(dev, dy0, mis.get("dy", 0)).t)
        assert np.array_equal(y.detach().cpu().numpy(), y_ref) and np.array_equal(x.grad.cpu().numpy(), dx_ref), (shape, k, mis)


# ---------------------------------------------------------------------------------------------------------
# output head and loss
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [5, 62, 129])
def test_log_softmax_misaligned(dev, V):
    """Rows and per-row bounds of test_gpu_kernels.test_log_softmax_argmax_edges_vs_oracle (Gaussian rows, exact ties, -inf entries, rows
    shifted by +-1e4; eps = 2^-23: log-probs 4 eps (|max z| + ln V + 1) + (V / 64 + 8) eps, dlogits 4 eps (max|g| + max p (V / 64 + 8) sum|g|)
    against log_softmax_bwd of the kernel's own log-probs), with the logits and the upstream gradient misaligned."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(V)
    rows = 23
    z = rs.standard_normal((rows, V)) * 3.0
    z[3:8] = np.round(z[3:8] / 2.0)
    for r in range(8, 12):
        z[r, rs.randint(0, V, size=max(1, V // 3))] = -np.inf
        z[r, rs.randint(0, V)] = 5.0
    z[12:15] += 1e4
    z[15:18] -= 1e4
    z = z.astype(np.float32)
    g = rs.standard_normal((rows, V)).astype(np.float32)
    eps = 2.0 ** -23
    fin = np.isfinite(z)
    with np.errstate(invalid="ignore"):
        lp_ref = R.log_softmax(z)
    zmax = np.abs(np.where(fin, z, 0.0)).max(axis=1)
    tol_lp = 4 * eps * (zmax + np.log(V) + 1.0) + (V / 64 + 8) * eps
    g64 = np.abs(g.astype(np.float64))
    for mis in offset_cases(["z", "g"]):
        zt = place(dev, z, mis.get("z", 0)).t.requires_grad_(True)
        lp = ops.log_softmax(zt)
        lp.backward(place(dev, g, mis.get("g", 0)).t)
        lp_k, dz = lp.detach().cpu().numpy(), zt.grad.cpu().numpy().astype(np.float64)
        assert not np.isnan(lp_k).any() and not np.isnan(dz).any(), ("NaN: a guard was read", V, mis)
        assert np.array_equal(np.isfinite(lp_k), fin) and np.all(lp_k[~fin] == -np.inf), (V, mis)
        err_lp = np.where(fin, np.abs(lp_k.astype(np.float64) - np.where(fin, lp_ref, 0.0)), 0.0).max(axis=1)
        assert np.all(err_lp <= tol_lp), (V, mis, (err_lp / tol_lp).max())
        p = np.exp(lp_k.astype(np.float64))
        tol_dz = 4 * eps * (g64.max(axis=1) + p.max(axis=1) * (V / 64 + 8) * g64.sum(axis=1))
        assert np.all(np.abs(dz - R.log_softmax_bwd(lp_k.astype(np.float64), g.astype(np.float64))).max(axis=1) <= tol_dz), (V, mis)
        assert np.array_equal(dz[~fin], g.astype(np.float64)[~fin]), (V, mis)


def test_ctc_loss_and_forced_align_misaligned(dev):
    """ops.ctc_loss with the log-probs and the per-utterance upstream gradient (reduction 'none') misaligned, against torch's CPU CTCLoss at
    the gates of test_gpu_kernels.test_ctc_vs_torch_cpu_random (loss relative 1e-5; gradient at the logits max-abs 2e-5 -- the gradient at
    the log-probs is taken through log_softmax's backward in float64 on both sides, which is what that test compares).
    ops.ctc_forced_align on the same misaligned log-probs: every output on its bits against test_ctc_align_host.align_ref, as test_ctc_align."""
    from ctc_pytorch_amd import ops
    from test_ctc_align_host import align_ref
    T, B, V = 40, 5, 13
    bt = synth.make_batch(seed=9, B=B, T=T, F=4, V=V, lab_lo=3, lab_hi=6)
    rs = np.random.RandomState(3)
    tg, tl, il = torch.from_numpy(bt["targets"]), torch.from_numpy(bt["tgt_len"]), torch.from_numpy(bt["lens"])
    zr = torch.from_numpy((2 * rs.standard_normal((T, B, V))).astype(np.float32)).requires_grad_(True)
    gw = (0.5 + rs.random_sample(B)).astype(np.float32)
    lpr = torch.log_softmax(zr, -1)
    nll_r = tnn.CTCLoss(reduction="none")(lpr, tg, il, tl)
    nll_r.backward(torch.from_numpy(gw))
    lp0 = lpr.detach().numpy()
    want = align_ref(lp0, bt["targets"], bt["lens"], bt["tgt_len"], 0)
    for mis in offset_cases(["lp", "g"]):
        lp = place(dev, lp0, mis.get("lp", 0)).t.requires_grad_(True)
        nll = ops.ctc_loss(lp, tg.to(dev), il.to(dev), tl.to(dev), reduction="none")
        nll.backward(place(dev, gw, mis.get("g", 0)).t)
        assert maxabs(nll, nll_r.detach()) < 1e-5 * float(nll_r.abs().max()), mis
        glp = lp.grad.cpu().numpy().astype(np.float64)
        assert not np.isnan(glp).any(), ("NaN: a guard was read", mis)
        assert maxabs(R.log_softmax_bwd(lp0.astype(np.float64), glp), zr.grad) < 2e-5, mis
        out = ops.ctc_forced_align(lp.detach(), tg.to(dev), il.to(dev), tl.to(dev), blank=0)
        for k in ("paths", "frame_scores", "scores", "ok", "starts", "ends"):
            a, c = np.ascontiguousarray(getattr(out, k).cpu().numpy()), np.ascontiguousarray(want[k])
            assert a.dtype == c.dtype and a.shape == c.shape, (k, mis)
            if a.dtype == np.float32:
                a, c = a.view(np.int32), c.view(np.int32)
            assert np.array_equal(a, c), (k, mis)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 5, 61, 10)])
def test_layout_conversions_misaligned(dev, shape):
    """ops.bctf_to_tbcf both ways through autograd and ops.contiguous on a strided view of a misaligned buffer: pure copies, exact against
    torch's own transposes."""
    from ctc_pytorch_amd import ops
    B, C, T, F = shape
    rs = np.random.RandomState(sum(shape))
    x0, dy0 = rs.standard_normal(shape).astype(np.float32), rs.standard_normal((T, B, C * F)).astype(np.float32)
    want = torch.from_numpy(x0).transpose(1, 2).reshape(B, T, C * F).transpose(0, 1).contiguous()
    dwant = torch.from_numpy(dy0).transpose(0, 1).reshape(B, T, C, F).transpose(1, 2).contiguous()
    for mis in offset_cases(["x", "dy"]):
        x = place(dev, x0, mis.get("x", 0)).t.requires_grad_(True)
        y = ops.bctf_to_tbcf(x)
        y.backward(place(dev, dy0, mis.get("dy", 0)).t)
        assert torch.equal(y.detach().cpu(), want) and torch.equal(x.grad.cpu(), dwant), (shape, mis)
        xs = place(dev, x0, mis.get("x", 0)).t.requires_grad_(True)
        view = xs.permute(3, 0, 2, 1)
        assert not view.is_contiguous()
        yc = ops.contiguous(view)
        gc = place(dev, rs.standard_normal(tuple(view.shape)).astype(np.float32), mis.get("dy", 0)).t
        yc.backward(gc)
        assert yc.is_contiguous() and torch.equal(yc.detach().cpu(), torch.from_numpy(x0).permute(3, 0, 2, 1).contiguous()), (shape, mis)
        assert torch.equal(xs.grad.cpu(), gc.cpu().permute(1, 3, 2, 0)), (shape, mis)


# ---------------------------------------------------------------------------------------------------------
# optimiser kernels on a misaligned slice: one rounding sequence on both paths -> bit-identical to the aligned call
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 1027])
def test_adam_and_clip_on_misaligned_slices_equal_aligned(dev, n):
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(n)
    p0, g0 = rs.standard_normal(n).astype(np.float32), (3.0 * rs.standard_normal(n)).astype(np.float32)

    def run(k):
        p, g, m, v = (Placed(dev, (n,), k) for _ in range(4))
        p.t.copy_(torch.from_numpy(p0).to(dev))
        g.t.copy_(torch.from_numpy(g0).to(dev))
        m.t.zero_()
        v.t.zero_()
        ops.adam_step(p.t, g.t, m.t, v.t, 1e-3, 0.9, 0.999, 1e-8, 5e-4, 1)
        p1 = p.t.clone()
        ctl = ops.new_clip_ctl(dev, step=1)
        norm = ops.grad_norm(g.t, 2.0, ctl=ctl).clone()
        ops.clip_control(ctl, 0.5, 1e-3, 0.9, 0.999, False)
        ops.adam_step_ex(p.t, g.t, m.t, v.t, 0.9, 0.999, 1e-8, 5e-4, ctl)
        g_before = g.t.clone()
        total = ops.clip_grad_norm_(g.t, 0.5).clone()
        torch.cuda.synchronize()
        assert all(q.guards_intact() for q in (p, g, m, v)), ("wrote outside the slice", n, k)
        assert torch.equal(norm, total)
        return [p.t.clone(), m.t.clone(), v.t.clone(), g.t.clone(), g_before, norm, p1]

    base = run(0)
    # references of the aligned tests: R.adam_step (test_adam_vs_oracle, 2e-6) and torch's clip_grad_norm_ expression (test_grad_clip)
    pr, _, _ = R.adam_step(p0.astype(np.float64), g0.astype(np.float64), np.zeros(n), np.zeros(n), 1, 1e-3, 5e-4)
    want_norm = float(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))
    assert maxabs(base[6], pr) < 2e-6
    assert abs(np.float32(float(base[5])) - np.float32(want_norm)) <= np.spacing(np.float32(want_norm))          # 1 ulp, as test_grad_clip
    # |g * coef| < 2 here: one float32 rounding (1.2e-7) on top of the coefficient's own 1-ulp error
    assert maxabs(base[3], g0.astype(np.float64) * min(1.0, 0.5 / (want_norm + 1e-6))) < 1e-6
    for k in (1, 2, 3):
        got = run(k)
        for a, b, what in zip(got, base, ("p", "m", "v", "clipped g", "g", "norm", "p after the plain step")):
            assert torch.equal(a, b), (what, n, k)


# ---------------------------------------------------------------------------------------------------------
# element-wise ops whose two paths share one rounding sequence: bit-identical to offset 0
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 1027])
def test_relu_and_dropout_misaligned_equal_aligned(dev, n):
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(n + 1)
    x0, dy0 = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)

    def run(k, fn):
        x = place(dev, x0, k).t.requires_grad_(True)
        ops._drop_counter[0] = 77
        y = fn(x)
        y.backward(place(dev, dy0, k).t)
        return y.detach().clone(), x.grad.clone()

    for fn, want in ((ops.relu, np.maximum(x0, 0.0)), (lambda t: ops.dropout(t, 0.3, True), None)):
        base = run(0, fn)
        if want is not None:
            assert np.array_equal(base[0].cpu().numpy(), want) and np.array_equal(base[1].cpu().numpy(), dy0 * (x0 > 0))
        for k in (1, 2, 3):
            got = run(k, fn)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), k


# ---------------------------------------------------------------------------------------------------------
# optim.FlatAdam: every parameter on 16 bytes, zero padding that stays zero
# ---------------------------------------------------------------------------------------------------------
ODD_CNN = [[(1, 3), (3, 3), (1, 2), (1, 1), None], [(3, 5), (3, 3), (1, 2), (1, 1), None]]


def _odd_model(which, nn_mod, relu, cls):
    """The two odd-sized models: 3 and 5 CNN channels in front of a 2 x 16 BiLSTM, and a 39-d input without CNN."""
    if which == "odd_cnn":
        rp = {"rnn_input_size": 40, "rnn_hidden_size": 16, "rnn_layers": 2, "rnn_type": nn_mod.LSTM, "bidirectional": True, "batch_norm": True}
        cp = {"batch_norm": True, "activate_function": relu, "layer": ODD_CNN}
        return cls(add_cnn=True, cnn_param=cp, rnn_param=rp, num_class=13, drop_out=0.0), 40
    rp = {"rnn_input_size": 39, "rnn_hidden_size": 16, "rnn_layers": 2, "rnn_type": nn_mod.LSTM, "bidirectional": True, "batch_norm": True}
    return cls(rnn_param=rp, num_class=13, drop_out=0.0), 39


def _padding_mask(opt):
    pad = torch.ones(opt.flat.numel(), dtype=torch.bool, device=opt.flat.device)
    for _, off, n, _ in opt._slices():
        pad[off:off + n] = False
    return pad


def _odd_pair(which, dev):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    m, F = _odd_model(which, nn, nn.ReLU, CTC_Model)
    ref, _ = _odd_model(which, tnn, tnn.ReLU, torch_cpu.TorchCpuCTCModel)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=91)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}
    m.load_state_dict(sd)
    ref.load_state_dict(sd)
    b = synth.make_batch(seed=1, B=3, T=61, F=F, V=13, lab_lo=3, lab_hi=6)
    return m.to(dev).train(), ref.train(), b


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("which", ["odd_cnn", "odd_input"])
def test_odd_sized_model_three_flat_adam_steps_vs_torch_cpu(dev, which, prec):
    """Three FlatAdam steps of a model whose parameter sizes are not multiples of 4 (before the padded layout: W_hh at an offset of 2 mod 4,
    refused by ctcn_rnn_fwd) against torch.optim.Adam on the torch-CPU restatement of the model (oracle/torch_cpu.py, the oracle of
    test_full_size_elementwise_vs_torch_cpu_oracle), at the gates of test_model_three_steps_golden."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.optim import FlatAdam
    ops.set_precision(prec)
    tol_act, tol_grad, tol_loss = (5e-5, 2e-4, 2e-5) if prec == 0 else (1e-3, 1e-3, 1e-3)
    m, ref, b = _odd_pair(which, dev)
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=5e-4)
    pad = _padding_mask(opt)
    assert int(pad.sum()) > 0 or which == "odd_input", "the odd channel counts need padding (39 inputs: odd leading dimensions only)"
    assert all(p.data_ptr() % 16 == 0 and p._ctcn_grad.data_ptr() % 16 == 0 for p in m.parameters())
    x, tg, tl = torch.from_numpy(b["x"]), torch.from_numpy(b["targets"]), torch.from_numpy(b["tgt_len"])
    B = x.shape[0]
    losses, rlosses = [], []
    for step in range(3):
        lp, rlp = m(x.to(dev)), ref(x)
        in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0)))
        loss = nn.CTCLoss(reduction="sum")(lp, tg.to(dev), in_len.to(dev), tl.to(dev)) / B
        rloss = tnn.CTCLoss(reduction="sum")(rlp, tg, in_len, tl) / B
        opt.zero_grad()
        ropt.zero_grad()
        loss.backward()
        rloss.backward()
        if step == 0:
            assert maxabs(lp, rlp) < tol_act
            rg = dict((k, p.grad) for k, p in ref.named_parameters())
            for k, p in m.named_parameters():
                if k.endswith("conv.bias"):         # identically zero in exact arithmetic (bias -> BatchNorm): magnitude only, as the golden test
                    assert float(p.grad.abs().max()) < 1e-4, k
                    continue
                assert rel_l2(p.grad, rg[k]) < tol_grad or maxabs(p.grad, rg[k]) < 1e-6, (k, rel_l2(p.grad, rg[k]))
        opt.step()
        ropt.step()
        losses.append(float(loss))
        rlosses.append(float(rloss))
    torch.cuda.synchronize()
    ops.check_health()
    assert np.allclose(losses, rlosses, rtol=tol_loss), (losses, rlosses)
    for t in (opt.flat, opt.grad, opt.m, opt.v):
        assert not bool(t[pad].any()), "a padding element moved"
    want_sd = ref.state_dict()
    for k, v in m.state_dict().items():
        want = want_sd[k]
        if "num_batches" in k:
            assert int(v) == int(want), k
        elif k.endswith("conv.bias") or (k.startswith("conv.") and k.endswith("running_mean")):
            assert maxabs(v, want) < 3.5e-3, k
        else:
            dv = (v.detach().cpu().double() - want.double()).abs()
            assert float(dv.max()) < 3.5e-3, k
            if prec == 0:
                assert float((dv > 5e-5).double().mean()) < 0.01, (k, float(dv.max()))
            else:
                assert rel_l2(v, want) < tol_grad or float(dv.max()) < 1e-5, (k, rel_l2(v, want))
    ops.set_precision(0)


RAGGED = [61, 20, 33]              # frames per utterance of the length-aware step (T = 61; labels of 3 .. 6 tokens fit 20 frames)


@pytest.mark.parametrize("which", ["odd_cnn", "odd_input"])
def test_odd_sized_model_clipped_and_length_aware_steps(dev, which):
    """One step with max_grad_norm (weight decay on), then one with ragged input_lengths whose padding holds noise of magnitude 1e4: against
    torch's clip_grad_norm_ + Adam on the packed CPU restatement (tests/packed_ref.py, the reference of test_length_mask.py; with full
    lengths it is the torch-CPU model).  Log-probs at the real frames at tol_act of test_model_three_steps_golden; the padding of the flat
    buffers stays zero through both steps."""
    import packed_ref
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.optim import FlatAdam
    m, _, b = _odd_pair(which, dev)
    ref, _ = _odd_model(which, tnn, tnn.ReLU, packed_ref.PackedCpuCTCModel)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    ref.train()
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4, max_grad_norm=0.05)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=5e-4)
    pad = _padding_mask(opt)
    # nn.utils.clip_grad_norm_ (the call of the reference's train script) finds the flat gradient of a padded layout: the library's norm kernel
    found = nn._flat_grad_of(list(m.parameters()))
    assert found is not None and found.data_ptr() == opt.grad.data_ptr() and found.numel() == opt.grad.numel()
    assert int(pad.sum()) > 0 or which == "odd_input"
    x, tg, tl = torch.from_numpy(b["x"]), torch.from_numpy(b["targets"]), torch.from_numpy(b["tgt_len"])
    B, T = x.shape[0], x.shape[1]
    noisy = x.clone()
    gen = torch.Generator().manual_seed(17)
    for i, n in enumerate(RAGGED):
        noisy[i, n:] = 1e4 * torch.randn(T - n, x.shape[2], generator=gen)
    for step, lens in enumerate((None, RAGGED)):
        if lens is None:
            lp, rlp = m(x.to(dev)), ref(x, [T] * B)
            in_len = torch.from_numpy(R.frames_from_fraction(b["frac"], lp.size(0)))
        else:
            lp, rlp = m(noisy.to(dev), input_lengths=lens), ref(noisy, lens)
            in_len = m.output_lengths(lens)
            assert in_len.tolist() == ref.output_lengths(lens).tolist() and in_len.tolist() != [int(lp.size(0))] * B
        loss = nn.CTCLoss(reduction="sum")(lp, tg.to(dev), in_len.to(dev), tl.to(dev)) / B
        rloss = tnn.CTCLoss(reduction="sum")(rlp, tg, in_len, tl) / B
        assert bool(torch.isfinite(lp).all())
        for i, n in enumerate(in_len.tolist() if lens is not None else [int(lp.size(0))] * B):
            assert maxabs(lp[:n, i], rlp[:n, i]) < 5e-5, (step, i)   # (tol_act of test_model_three_steps_golden, precision 0)
        assert abs(float(loss) - float(rloss)) < 2e-5 * abs(float(rloss)), (step, float(loss), float(rloss))      # (its tol_loss)
        opt.zero_grad()
        ropt.zero_grad()
        loss.backward()
        rloss.backward()
        rg = dict((k, p.grad) for k, p in ref.named_parameters())
        for k, p in m.named_parameters():      # both steps' gradients, the ragged one against the packed reference: tol_grad of test_model_three_steps_golden
            if k.endswith("conv.bias"):        # identically zero in exact arithmetic (bias -> BatchNorm): magnitude only, as the golden test
                assert float(p.grad.abs().max()) < 1e-4, (step, k)
            else:
                assert rel_l2(p.grad, rg[k]) < 2e-4 or maxabs(p.grad, rg[k]) < 1e-6, (step, k, rel_l2(p.grad, rg[k]))
        if step == 0:
            # the same norm from nn.utils.clip_grad_norm_ with a bound that does not clip: 1 ulp of the float32 norm, as test_grad_clip
            unclipped = opt.grad.clone()
            total = nn.utils.clip_grad_norm_(m.parameters(), 1e9)
            want_norm = np.float32(np.sqrt(float((unclipped.double() ** 2).sum())))
            assert abs(np.float32(float(total)) - want_norm) <= np.spacing(want_norm), (float(total), float(want_norm))
            assert torch.equal(opt.grad, unclipped)
        rnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05)
        opt.step()
        ropt.step()
        assert abs(float(opt.last_grad_norm) - float(rnorm)) < 2e-4 * float(rnorm), (step, float(opt.last_grad_norm), float(rnorm))
        assert float(rnorm) > 0.05, "the clip must be active"
    torch.cuda.synchronize()
    ops.check_health()
    for t in (opt.flat, opt.grad, opt.m, opt.v):
        assert not bool(t[pad].any()), "a padding element moved"
    want_sd = ref.state_dict()
    for k, v in m.state_dict().items():
        if "num_batches" in k:
            continue
        dv = (v.detach().cpu().double() - want_sd[k].double()).abs()
        assert float(dv.max()) < 3.5e-3, k                           # no entry beyond 3 steps * lr (test_model_three_steps_golden)
        if not (k.endswith("conv.bias") or (k.startswith("conv.") and k.endswith("running_mean"))):
            assert float((dv > 5e-5).double().mean()) < 0.01, (k, float(dv.max()))      # (its precision-0 gate on the parameters)


def test_flat_adam_state_dict_round_trip_on_a_padded_layout(dev):
    """state_dict() of a padded layout is torch.optim.Adam's per-parameter form (no padding in it) and loads back bit for bit, into torch's
    Adam as well."""
    import copy
    from ctc_pytorch_amd.optim import FlatAdam
    m, _, _ = _odd_pair("odd_cnn", dev)
    m2 = copy.deepcopy(m)
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4)
    pad = _padding_mask(opt)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for _ in range(2):
        opt.zero_grad()
        for p in m.parameters():
            p.grad.copy_(torch.randn(p.shape, generator=gen).to(dev))
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    params = list(m.parameters())
    assert sorted(sd["state"]) == list(range(len(params)))
    assert all(sd["state"][i]["exp_avg"].shape == p.shape and float(sd["state"][i]["step"]) == 2.0 for i, p in enumerate(params))
    m_was, v_was = opt.m.clone(), opt.v.clone()
    opt.m.fill_(3.0)
    opt.v.fill_(3.0)
    opt.load_state_dict(sd)
    assert torch.equal(opt.m, m_was) and torch.equal(opt.v, v_was) and opt.step_count == 2
    assert not bool(opt.m[pad].any()) and not bool(opt.v[pad].any())
    ta = torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=5e-4)
    ta.load_state_dict(sd)
    for i, p in enumerate(m2.parameters()):
        assert torch.equal(ta.state[p]["exp_avg"], sd["state"][i]["exp_avg"])
