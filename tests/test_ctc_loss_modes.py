"""nn.CTCLoss's whole contract on the HIP kernels (blank, reduction, zero_infinity, concatenated targets, unbatched input) against
torch.nn.functional.ctc_loss on the CPU in float64 and float32, and the old entry points against the new ones bit for bit.

Tolerances are test_gpu_kernels.py's test_ctc_vs_torch_cpu_random ones: loss rel <= 1e-5, gradient max-abs <= max(2e-5, 3 x the
distance of torch's own float32 result to float64)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ctc_pytorch_amd.testing import synth

pytestmark = pytest.mark.gpu


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


def _maxabs(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float64))
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b, dtype=np.float64))
    return float((a - b).abs().max()) if a.numel() else 0.0


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().cpu().view(torch.int32), b.detach().cpu().view(torch.int32))


def _ragged_batch(blank, T=200, B=16, V=62, seed=9):
    """synth's ragged lengths, labels drawn from the classes other than `blank`, and hand-set rows: an empty label (0), an infeasible
    utterance (1: input shorter than the label), a long run of repeats (2), an infeasible run of repeats (3: needs 2L - 1 frames),
    an input shorter than T (4)."""
    b = synth.make_batch(seed=seed, B=B, T=T, F=4, V=V, lab_lo=10, lab_hi=60)
    rs = np.random.RandomState(seed + 100 * blank)
    tl, il = b["tgt_len"].copy(), b["lens"].copy()
    tl[0] = 0
    tl[1], il[1] = 30, 20
    tl[2], il[2] = 40, T
    tl[3], il[3] = 12, 20
    tl[4], il[4] = 15, T // 3
    Lmax = int(tl.max())
    lab = rs.randint(0, V - 1, size=(B, Lmax))
    lab = lab + (lab >= blank)                                    # every class but the blank
    tg = np.zeros((B, Lmax), dtype=np.int64)
    for i in range(B):
        tg[i, :tl[i]] = lab[i, :tl[i]]
    tg[2, :40] = tg[2, 0]
    tg[3, :12] = tg[3, 0]
    logits = (2 * rs.standard_normal((T, B, V))).astype(np.float32)
    return logits, tg, il.astype(np.int64), tl.astype(np.int64)


def _torch_cpu(logits, tg, il, tl, blank, reduction, zero_infinity, w, dtype):
    x = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    loss = F.ctc_loss(torch.log_softmax(x, -1), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl), blank=blank,
                      reduction=reduction, zero_infinity=zero_infinity)
    (loss * w.to(dtype)).sum().backward() if reduction == "none" else loss.backward()
    return loss.detach(), x.grad


def _ours(dev, logits, tg, il, tl, blank, reduction, zero_infinity, w):
    from ctc_pytorch_amd import nn, ops
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    loss = nn.CTCLoss(blank=blank, reduction=reduction, zero_infinity=zero_infinity)(
        ops.log_softmax(x), torch.from_numpy(tg).to(dev), torch.from_numpy(il).to(dev), torch.from_numpy(tl).to(dev))
    (loss * w.to(dev)).sum().backward() if reduction == "none" else loss.backward()
    return loss.detach().cpu(), x.grad.cpu()


def _check_against_torch(loss, grad, logits, tg, il, tl, blank, reduction, zero_infinity, w):
    l64, g64 = _torch_cpu(logits, tg, il, tl, blank, reduction, zero_infinity, w, torch.float64)
    l32, g32 = _torch_cpu(logits, tg, il, tl, blank, reduction, zero_infinity, w, torch.float32)
    assert loss.shape == l64.shape
    fin = torch.isfinite(l64)
    assert torch.equal(torch.isfinite(loss), fin) and torch.equal(torch.isinf(loss), torch.isinf(l64))
    rel = ((loss.double()[fin] - l64[fin]).abs() / l64[fin].abs().clamp_min(1e-30)).max() if bool(fin.any()) else torch.zeros(())
    assert float(rel) <= 1e-5, float(rel)
    nan = torch.isnan(g32)
    assert torch.equal(torch.isnan(grad), nan) and torch.equal(torch.isnan(g64), nan)
    ok = ~nan
    err, err32 = _maxabs(grad[ok], g64[ok]), _maxabs(g32[ok], g64[ok])
    assert err <= max(2e-5, 3.0 * err32), (err, err32)
    return l64, g64


@pytest.mark.parametrize("blank", [0, 1, 61])
@pytest.mark.parametrize("zero_infinity", [False, True])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_ctc_modes_vs_torch_cpu(dev, reduction, zero_infinity, blank):
    logits, tg, il, tl = _ragged_batch(blank)
    B = tg.shape[0]
    w = torch.linspace(0.25, 2.0, B)                   # 'none': a non-uniform per-utterance weighting
    loss, grad = _ours(dev, logits, tg, il, tl, blank, reduction, zero_infinity, w)
    _check_against_torch(loss, grad, logits, tg, il, tl, blank, reduction, zero_infinity, w)
    infeasible = [1, 3]
    if zero_infinity:
        assert bool(torch.isfinite(loss).all())
        if reduction == "none":
            assert all(float(loss[i]) == 0.0 for i in infeasible)
        assert bool((grad[:, infeasible] == 0).all()) and bool(torch.isfinite(grad).all())
    else:
        assert bool(torch.isinf(loss).any())
        assert bool(torch.isnan(grad[:, infeasible]).any()) and bool(torch.isfinite(grad[:, [0, 2, 4]]).all())


def test_ctc_long_labels_mean_blank_last(dev):
    """L ~ 2 000 (S = 4 001: the sixteen-states-per-thread lattice), blank = V - 1, 'mean', against float64."""
    T, B, V = 4300, 2, 40
    rs = np.random.RandomState(77)
    tl = np.array([2000, 1700], dtype=np.int64)
    tg = rs.randint(0, V - 1, size=(B, 2000)).astype(np.int64)
    tg[1, 1700:] = 0
    il = np.array([T, 3900], dtype=np.int64)
    logits = (1.5 * rs.standard_normal((T, B, V))).astype(np.float32)
    loss, grad = _ours(dev, logits, tg, il, tl, V - 1, "mean", False, None)
    l64, _ = _check_against_torch(loss, grad, logits, tg, il, tl, V - 1, "mean", False, None)
    assert bool(torch.isfinite(l64))


@pytest.mark.parametrize("lengths_on", ["host", "device"])
def test_ctc_concatenated_targets_bit_identical_to_padded(dev, lengths_on):
    from ctc_pytorch_amd import nn, ops
    logits, tg, il, tl = _ragged_batch(blank=1)
    flat = torch.from_numpy(np.concatenate([tg[i, :tl[i]] for i in range(tg.shape[0])]))
    lp = ops.log_softmax(torch.from_numpy(logits).to(dev))
    outs = []
    for targets, tlen in ((torch.from_numpy(tg).to(dev), torch.from_numpy(tl).to(dev)),
                          (flat.to(dev), tl.tolist() if lengths_on == "host" else torch.from_numpy(tl).to(dev))):
        x = lp.detach().clone().requires_grad_(True)
        ilen = il.tolist() if lengths_on == "host" else torch.from_numpy(il).to(dev)
        nll = nn.CTCLoss(blank=1, reduction="none")(x, targets, ilen, tlen)
        nll.backward(torch.linspace(0.5, 1.5, tg.shape[0], device=dev))
        x2 = lp.detach().clone().requires_grad_(True)
        m = nn.CTCLoss(blank=1, reduction="mean", zero_infinity=True)(x2, targets, ilen, tlen)
        m.backward()
        outs.append((nll.detach(), x.grad, m.detach(), x2.grad))
    for a, b in zip(*outs):
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def _abi_old_vs_new(dev, lp, tg, il, tl):
    """The four old entry points and the new ones on the same inputs, raw through the C ABI: nll, alpha, beta, alpha + beta and the
    gradient bit for bit, and the loss of nn.CTCLoss(reduction='sum') (blank 0) against ctcn_sum_f32 over the old nll."""
    from ctc_pytorch_amd import _lib, nn
    T, B, V = lp.shape
    Lmax = tg.shape[1]
    L, st = _lib.lib(), _lib.stream_ptr()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    Z = lambda: torch.zeros((T, B, 2 * Lmax + 1), device=dev)
    gs = torch.full((), 1.0 / B, device=dev)
    # old
    a1, n1, g1 = Z(), torch.empty(B, device=dev), torch.zeros_like(lp)
    _lib.check(L.ctcn_ctc_fwd(P(lp), P(tg), P(il), P(tl), P(a1), P(n1), T, B, V, Lmax, st), "ctc_fwd")
    alpha_only = a1.clone()
    _lib.check(L.ctcn_ctc_bwd(P(lp), P(tg), P(il), P(tl), P(a1), P(n1), P(gs), P(g1), T, B, V, Lmax, st), "ctc_bwd")
    a2, b2, n2, g2 = Z(), Z(), torch.empty(B, device=dev), torch.zeros_like(lp)
    _lib.check(L.ctcn_ctc_fwd_both(P(lp), P(tg), P(il), P(tl), P(a2), P(b2), P(n2), T, B, V, Lmax, st), "ctc_fwd_both")
    _lib.check(L.ctcn_ctc_grad(P(lp), P(tg), P(il), P(tl), P(a2), P(b2), P(n2), P(gs), P(g2), T, B, V, Lmax, st), "ctc_grad")
    s_old = torch.empty((), device=dev)
    _lib.check(L.ctcn_sum_f32(P(n2), P(s_old), B, st), "sum_f32")
    # new
    a3, n3 = Z(), torch.empty(B, device=dev)
    _lib.check(L.ctcn_ctc_fwd_ex(P(lp), P(tg), P(il), P(tl), P(a3), None, P(n3), T, B, V, Lmax, 0, st), "ctc_fwd_ex")
    a4, b4, n4, g4, g5 = Z(), Z(), torch.empty(B, device=dev), torch.zeros_like(lp), torch.zeros_like(lp)
    _lib.check(L.ctcn_ctc_fwd_ex(P(lp), P(tg), P(il), P(tl), P(a4), P(b4), P(n4), T, B, V, Lmax, 0, st), "ctc_fwd_ex")
    _lib.check(L.ctcn_ctc_grad_ex(P(lp), P(tg), P(il), P(tl), P(a4), P(b4), P(n4), P(gs), 0, 2, 0, 0, P(g4), T, B, V, Lmax, st), "ctc_grad_ex")
    _lib.check(L.ctcn_ctc_grad_ex(P(lp), P(tg), P(il), P(tl), P(a1), None, P(n1), P(gs), 0, 2, 0, 0, P(g5), T, B, V, Lmax, st), "ctc_grad_ex")
    s_new, v_new = torch.empty((), device=dev), torch.empty(B, device=dev)
    _lib.check(L.ctcn_ctc_reduce(P(n4), P(tl), P(s_new), B, 2, 0, st), "ctc_reduce")
    _lib.check(L.ctcn_ctc_reduce(P(n4), P(tl), P(v_new), B, 0, 0, st), "ctc_reduce")
    torch.cuda.synchronize()
    assert _same_bits(n1, n2) and _same_bits(n1, n3) and _same_bits(n2, n4) and _same_bits(v_new, n2)
    assert _same_bits(alpha_only, a2) and _same_bits(a3, a2) and _same_bits(a4, a2) and _same_bits(b4, b2)
    assert _same_bits(a1, a2 + b2)
    assert _same_bits(g1, g2) and _same_bits(g4, g2) and _same_bits(g5, g2)
    assert _same_bits(s_new, s_old)
    # the autograd path: nn.CTCLoss(reduction='sum') is the sum of the old nll and its gradient the old one, bit for bit
    x = lp.detach().clone().requires_grad_(True)
    loss = nn.CTCLoss(reduction="sum")(x, tg, il, tl)
    loss.backward(gs)
    assert _same_bits(loss.detach(), s_old) and _same_bits(x.grad, g2)
    nll = nn.CTCLoss(reduction="none")(lp, tg, il, tl)
    assert _same_bits(nll, n2)
    return n2, g2


def test_ctc_old_entry_points_unchanged_cfg2_shape(dev):
    from ctc_pytorch_amd import ops
    T, B, V = 800, 32, 62
    b = synth.make_batch(seed=1, B=B, T=T, F=4, V=V, lab_lo=30, lab_hi=60, full_length=True)
    rs = np.random.RandomState(12)
    lp = ops.log_softmax(torch.from_numpy((2 * rs.standard_normal((T, B, V))).astype(np.float32)).to(dev)).detach()
    il = torch.from_numpy(b["lens"]).to(dev)
    il[-1] = 25                                        # one infeasible utterance: +inf and its NaN rows must match too
    _abi_old_vs_new(dev, lp, torch.from_numpy(b["targets"]).to(dev), il, torch.from_numpy(b["tgt_len"]).to(dev))


def test_ctc_old_entry_points_unchanged_golden_batch(dev):
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ctc_loss.npz"))
    lp = torch.from_numpy(z["lp"]).to(dev)
    tg, tl = torch.from_numpy(z["targets"]).to(dev), torch.from_numpy(z["tgt_len"]).to(dev)
    for key in ("in_len", "in_len_inf"):
        n2, _ = _abi_old_vs_new(dev, lp, tg, torch.from_numpy(z[key]).to(dev), tl)
        if key == "in_len":
            assert np.allclose(n2.cpu().numpy(), z["nll"], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_ctc_unbatched_input(dev, reduction):
    from ctc_pytorch_amd import nn, ops
    T, V = 50, 12
    rs = np.random.RandomState(5)
    logits = (1.5 * rs.standard_normal((T, V))).astype(np.float32)
    tg = torch.tensor([3, 3, 7, 1, 9])
    xr = torch.from_numpy(logits).double().requires_grad_(True)
    lr = F.ctc_loss(torch.log_softmax(xr, -1), tg, torch.tensor(T - 4), torch.tensor(5), blank=2, reduction=reduction)
    lr.backward()
    for il, tl in ((torch.tensor(T - 4), torch.tensor(5)), ([T - 4], [5]), (torch.tensor([T - 4], device=dev), torch.tensor([5], device=dev))):
        x = torch.from_numpy(logits).to(dev).requires_grad_(True)
        loss = nn.CTCLoss(blank=2, reduction=reduction)(ops.log_softmax(x), tg.to(dev), il, tl)
        assert loss.dim() == 0
        loss.backward()
        assert abs(float(loss) - float(lr)) / abs(float(lr)) <= 1e-5
        assert _maxabs(x.grad, xr.grad) <= 2e-5


@pytest.mark.parametrize("prec,tol", [(0, 1e-4), (1, 5e-4)])
def test_ctc_model_trains_with_torch_default_ctcloss(dev, prec, tol):
    """A small CTC_Model (BiLSTM 2 x 32) under nn.CTCLoss() at its defaults ('mean'), against the torch-CPU model with the same weights in
    float64 under torch.nn.CTCLoss()."""
    import torch.nn as tnn
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from oracle import np_ref, torch_cpu
    ops.set_precision(prec)
    V = 62
    b = synth.make_batch(seed=3, B=6, T=60, F=40, V=V, lab_lo=5, lab_hi=15)
    rp = {"rnn_input_size": 40, "rnn_hidden_size": 32, "rnn_layers": 2, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    model = CTC_Model(rnn_param=rp, num_class=V, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=5)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}
    model.load_state_dict(sd)
    model = model.to(dev).train()
    ref = torch_cpu.TorchCpuCTCModel(rnn_param=dict(rp, rnn_type=tnn.LSTM), num_class=V, drop_out=0.0)
    ref.load_state_dict(sd)
    ref = ref.double().train()
    x = torch.from_numpy(b["x"])
    tg, tl = torch.from_numpy(b["targets"]), torch.from_numpy(b["tgt_len"])
    out = model(x.to(dev))
    in_len = torch.from_numpy(np_ref.frames_from_fraction(b["frac"], out.size(0)))
    loss = nn.CTCLoss()(out, tg.to(dev), in_len.to(dev), tl.to(dev))
    loss.backward()
    loss_ref = tnn.CTCLoss()(ref(x.double()), tg, in_len, tl)
    loss_ref.backward()
    assert abs(float(loss) - float(loss_ref)) / abs(float(loss_ref)) <= 1e-5
    got = dict(model.named_parameters())
    for k, p in ref.named_parameters():
        g, r = got[k].grad.double().cpu(), p.grad
        assert float((g - r).norm() / r.norm().clamp_min(1e-30)) <= tol, k


def test_ctc_modes_deterministic(dev):
    logits, tg, il, tl = _ragged_batch(blank=1)
    r1 = _ours(dev, logits, tg, il, tl, 1, "mean", True, None)
    r2 = _ours(dev, logits, tg, il, tl, 1, "mean", True, None)
    assert _same_bits(r1[0], r2[0]) and _same_bits(r1[1], r2[1])
