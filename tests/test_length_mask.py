"""Length-aware forward / backward on the GPU (CTC_Model.forward(input_lengths=)): padding reaches no BatchNorm statistic, no recurrence
and no gradient.  Tolerances: the project's gates(prec, 2e-5, 4e-4, 1e-5) of test_full_size_elementwise_vs_torch_cpu_oracle (precision 1:
1e-3), conv.bias gradients excluded as there (identically zero in exact arithmetic: a bias feeding BatchNorm).  Every ragged batch holds
a full-length utterance and one near the shortest the front-end allows."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as tnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref  # noqa: E402
from bn_ref import _valid  # noqa: E402  (the validity rule of include/ctcn.h)
from ctc_pytorch_amd.testing import synth  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
CNN2 = [[(1, 4), (3, 3), (1, 2), (1, 1), None], [(4, 4), (3, 3), (2, 2), (1, 1), None]]
FAMILIES = [(cell, cnn) for cell in ("LSTM", "GRU", "RNN") for cnn in (False, True)]
LENS = [40, 3, 17, 40, 9, 26]                       # T = 40; 3 frames leave 2 behind the stride-2 front-end


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def gates(prec, strict_act, strict_grad, strict_loss):
    return (strict_act, strict_grad, strict_loss) if prec == 0 else (1e-3, 1e-3, 1e-3)


def maxabs(a, b):
    a, b = (t.detach().cpu().double() for t in (a, b))
    return float((a - b).abs().max()) if a.numel() else 0.0


def rel_l2(a, b):
    a, b = (t.detach().cpu().double() for t in (a, b))
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def build(cell, cnn, dev, F=12, H=16, L=3, V=9, drop=0.0, seed=91, layers=CNN2, reference=False):
    """(HIP model on dev, packed CPU reference or None) from one seeded state dict."""
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    rp = {"rnn_input_size": F, "rnn_hidden_size": H, "rnn_layers": L, "rnn_type": getattr(nn, cell), "bidirectional": True, "batch_norm": True}
    cp = {"batch_norm": True, "activate_function": nn.ReLU, "layer": layers} if cnn else None
    m = CTC_Model(add_cnn=cnn, cnn_param=cp, rnn_param=rp, num_class=V, drop_out=drop)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=seed)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}
    m.load_state_dict(sd)
    ref = None
    if reference:
        ref = packed_ref.PackedCpuCTCModel(add_cnn=cnn, cnn_param=dict(cp, activate_function=tnn.ReLU) if cnn else None,
                                           rnn_param=dict(rp, rnn_type=getattr(tnn, cell)), num_class=V, drop_out=drop)
        ref.load_state_dict(sd)
    return m.to(dev), ref


def batch(lens, T, F, V, out_lens, seed=5):
    """x (B,T,F) zero-padded, targets without adjacent repeats (feasible whenever tgt_len <= frames), tgt_len <= out_len / 3."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((len(lens), T, F)).astype(np.float32)
    for b, l in enumerate(lens):
        x[b, l:] = 0.0
    tl = np.array([max(1, int(n) // 3) for n in out_lens], dtype=np.int64)
    tg = np.zeros((len(lens), int(tl.max())), dtype=np.int64)
    for b in range(len(lens)):
        tg[b, :tl[b]] = 1 + (np.arange(tl[b]) + rs.randint(0, V - 1)) % (V - 1)
    return torch.from_numpy(x), torch.from_numpy(tg), torch.from_numpy(tl)


def fill_padding(x, lens, kind, seed=17):
    x = x.clone()
    g = torch.Generator().manual_seed(seed)
    for b, l in enumerate(lens):
        n = x.shape[1] - l
        if kind == "noise":
            x[b, l:] = 1e4 * torch.randn(n, x.shape[2], generator=g)
        elif kind == "nan":
            x[b, l:] = float("nan")
            x[b, l::2] = float("inf")
    return x


def step(m, x, lens, tg, tl, dev, masked=True):
    """forward + CTC (sum / B) + backward; returns (log-probs, loss, {name: grad})."""
    from ctc_pytorch_amd import nn
    m.zero_grad(set_to_none=True)
    lp = m(x.to(dev), input_lengths=lens) if masked else m(x.to(dev))
    out_len = m.output_lengths(lens)
    loss = nn.CTCLoss(reduction="sum")(lp, tg.to(dev), out_len.to(dev), tl.to(dev)) / x.shape[0]
    loss.backward()
    torch.cuda.synchronize()
    return lp.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def ref_step(ref, x, lens, tg, tl):
    before = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    try:
        ref.zero_grad(set_to_none=True)
        lp = ref(x, lens)
        loss = tnn.CTCLoss(reduction="sum")(lp, tg, ref.output_lengths(lens), tl) / x.shape[0]
        loss.backward()
    finally:
        torch.set_num_threads(before)
    return lp.detach(), float(loss), {k: p.grad.detach().clone() for k, p in ref.named_parameters()}


# ---- 1. what the padding holds is invisible, bit for bit -----------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("mode", ["train", "train_dropout", "eval"])
@pytest.mark.parametrize("cell,cnn", FAMILIES)
def test_padding_content_is_invisible_bit_for_bit(dev, cell, cnn, mode, prec):
    """Same model, lengths, B and T; the padded frames of x hold zeros, large finite noise, or NaN / Inf: out[:len_b, b], the loss, every
    parameter gradient and the BatchNorm running statistics after the step are bit-identical.  (Without lengths the padding enters the
    statistics and the reverse recurrence, and NaN poisons everything.)"""
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    T, F, V = max(LENS), 12, 9
    runs = []
    start = ops._drop_counter[0]
    for kind in ("zeros", "noise", "nan"):
        torch.manual_seed(0)
        ops._drop_counter[0] = start                                     # the same dropout stream for the three runs
        m, _ = build(cell, cnn, dev, drop=0.2 if mode == "train_dropout" else 0.0)
        out_len = m.output_lengths(LENS)
        x, tg, tl = batch(LENS, T, F, V, out_len)
        x = fill_padding(x, LENS, kind)
        if mode == "eval":
            m.eval()
            with torch.no_grad():
                lp = m(x.to(dev), input_lengths=LENS)
            torch.cuda.synchronize()
            loss, grads = torch.zeros(()), {}
        else:
            m.train()
            lp, loss, grads = step(m, x, LENS, tg, tl, dev)
        ops.check_health()
        assert bool(torch.isfinite(lp).all()), kind
        stats = {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
        runs.append((lp, loss, grads, stats))
    lp0, loss0, g0, s0 = runs[0]
    for kind, (lp, loss, g, s) in zip(("noise", "nan"), runs[1:]):
        for b, n in enumerate(m.output_lengths(LENS).tolist()):
            assert torch.equal(lp[:n, b], lp0[:n, b]), (kind, b)
        assert torch.equal(lp, lp0), kind                                # (the padded output frames too: log_softmax(0))
        assert torch.equal(loss.cpu(), loss0.cpu()), (kind, float(loss), float(loss0))
        for k in g0:
            assert torch.equal(g[k], g0[k]), (kind, k)
        for k in s0:
            assert torch.equal(s[k], s0[k]), (kind, k)
    if mode != "eval":
        assert float(loss0) > 0 and all(bool(torch.isfinite(v).all()) for v in g0.values())
        assert all(int(v) == 1 for k, v in s0.items() if "num_batches" in k)


# ---- 2. against the packed CPU reference ----------------------------------------------------------------------------
def _compare_with_reference(m, ref, x, lens, tg, tl, dev, prec, tag):
    tol_act, tol_grad, tol_loss = gates(prec, 2e-5, 4e-4, 1e-5)
    lp, loss, grads = step(m, x, lens, tg, tl, dev)
    lp_r, loss_r, grads_r = ref_step(ref, x, lens, tg, tl)
    out_len = m.output_lengths(lens).tolist()
    assert out_len == ref.output_lengths(lens).tolist()
    e_lp = max(maxabs(lp[:n, b], lp_r[:n, b]) for b, n in enumerate(out_len))
    e_loss = abs(float(loss) - loss_r) / abs(loss_r)
    errs = {k: rel_l2(grads[k], grads_r[k]) for k in grads if not k.endswith("conv.bias")}
    worst = max((v, k) for k, v in errs.items())
    sd, sd_r = m.state_dict(), ref.state_dict()
    # running statistics: a mean of activations is held to the activation gate (max-abs); a variance is a second moment, summed like a
    # gradient: rel-L2 at the gradient gate
    e_mean = max(maxabs(sd[k], sd_r[k]) for k in sd if k.endswith("running_mean"))
    e_var = max(rel_l2(sd[k], sd_r[k]) for k in sd if k.endswith("running_var"))
    print("\n[%s prec %d] max|dlp| %.3e  loss rel %.3e  grad rel-L2 worst %.3e (%s)  running mean %.3e var %.3e" % (
        tag, prec, e_lp, e_loss, worst[0], worst[1], e_mean, e_var))
    assert e_lp < tol_act, e_lp
    assert e_loss < tol_loss, e_loss
    assert worst[0] < tol_grad, worst
    assert e_mean < tol_act and e_var < tol_grad, (e_mean, e_var)
    for k in sd:
        if "num_batches" in k:
            assert int(sd[k]) == int(sd_r[k]) == 1, k


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell,cnn", FAMILIES)
def test_training_step_against_packed_reference_small(dev, cell, cnn, prec):
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    m, ref = build(cell, cnn, dev, reference=True)
    m.train(), ref.train()
    x, tg, tl = batch(LENS, max(LENS), 12, 9, m.output_lengths(LENS))
    x = fill_padding(x, LENS, "noise")
    _compare_with_reference(m, ref, x, LENS, tg, tl, dev, prec, "%s cnn=%s" % (cell, cnn))
    ops.check_health()


@pytest.mark.parametrize("prec", [0, 1])
def test_training_step_against_packed_reference_cfg2(dev, prec):
    """The cfg2 shape (B 32, T 800, 4 x 320 BiLSTM) with lengths drawn like bench.py's epoch_loop_ragged (U{T/4 .. T}); the persistent
    recurrences run it."""
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    c = json.load(open(os.path.join(G, "large_checksums.json")))["cfg2"]["shape"]
    rs = np.random.RandomState(11)
    lens = [int(rs.randint(c["T"] // 4, c["T"] + 1)) for _ in range(c["B"])]
    lens[0], lens[1] = c["T"], 1
    m, ref = build(c["rnn"], c["cnn"], dev, F=40, H=c["H"], L=c["L"], V=c["V"], reference=True)
    m.train(), ref.train()
    x, tg, tl = batch(lens, c["T"], 40, c["V"], m.output_lengths(lens))
    tl = torch.clamp(tl, max=60)
    tg = tg[:, :60].contiguous()
    x = fill_padding(x, lens, "noise")
    _compare_with_reference(m, ref, x, lens, tg, tl, dev, prec, "cfg2 ragged")
    ops.check_health()
    assert ops.rnn_last_kernels()[0] in ("rnn_fwd_tagged", "rnn_fwd_persist") and ops.rnn_last_kernels()[1] in (
        "rnn_bwd_scatter2", "rnn_bwd_scatter", "rnn_bwd_persist"), ops.rnn_last_kernels()


# ---- 3. an utterance does not depend on its batch -------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell,cnn", FAMILIES)
def test_eval_utterance_is_independent_of_its_batch(dev, cell, cnn, prec):
    """Eval mode: utterance b of a ragged (zero-padded) batch == the same utterance alone (B = 1, T = len_b) at the activation gate.  Control:
    the same comparison without input_lengths exceeds the gate -- these inputs see the defect (the forward direction's state runs on
    through the padding, and the next layer's reverse direction starts from it)."""
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    tol_act = gates(prec, 2e-5, 4e-4, 1e-5)[0]
    m, _ = build(cell, cnn, dev)
    m.eval()
    T = max(LENS)
    x, _, _ = batch(LENS, T, 12, 9, m.output_lengths(LENS))
    out_len = m.output_lengths(LENS).tolist()
    with torch.no_grad():
        masked = m(x.to(dev), input_lengths=LENS)
        plain = m(x.to(dev))
        e_masked = e_plain = 0.0
        for b, l in enumerate(LENS):
            alone = m(x[b:b + 1, :l].contiguous().to(dev))
            assert alone.shape[0] == out_len[b]
            e_masked = max(e_masked, maxabs(masked[:out_len[b], b], alone[:, 0]))
            e_plain = max(e_plain, maxabs(plain[:out_len[b], b], alone[:, 0]))
    ops.check_health()
    print("\n[%s cnn=%s prec %d] vs alone: with lengths %.3e, without %.3e" % (cell, cnn, prec, e_masked, e_plain))
    assert e_masked < tol_act, e_masked
    assert e_plain > tol_act, e_plain


# ---- 4. padded output frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell,cnn", FAMILIES)
def test_padded_output_frames_are_uniform(dev, cell, cnn, prec):
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    tol_act = gates(prec, 2e-5, 4e-4, 1e-5)[0]
    m, _ = build(cell, cnn, dev)
    m.train()
    x, _, _ = batch(LENS, max(LENS), 12, 9, m.output_lengths(LENS))
    lp = m(fill_padding(x, LENS, "nan").to(dev), input_lengths=LENS).detach().cpu()
    assert bool(torch.isfinite(lp).all())
    seen = 0
    for b, n in enumerate(m.output_lengths(LENS).tolist()):
        pad = lp[n:, b]
        seen += pad.shape[0]
        if pad.numel():
            assert bool((pad == pad[:, :1]).all()), b
            assert float((pad + np.log(lp.shape[-1])).abs().max()) < tol_act, b
    assert seen > 0


# ---- 5. full lengths == the unmasked path ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell,cnn", FAMILIES)
def test_full_lengths_agree_with_unmasked_path(dev, cell, cnn, prec):
    from ctc_pytorch_amd import ops
    ops.set_precision(prec)
    tol_act, tol_grad, tol_loss = gates(prec, 2e-5, 4e-4, 1e-5)
    B, T = 6, 40
    lens = [T] * B
    runs = []
    for masked in (True, False):
        m, _ = build(cell, cnn, dev)
        m.train()
        x, tg, tl = batch(lens, T, 12, 9, m.output_lengths(lens))
        runs.append(step(m, x, lens, tg, tl, dev, masked=masked) + ({k: v.clone() for k, v in m.state_dict().items() if "running" in k},))
    (lp, loss, g, s), (lp0, loss0, g0, s0) = runs
    bitwise = torch.equal(lp, lp0) and all(torch.equal(g[k], g0[k]) for k in g) and all(torch.equal(s[k], s0[k]) for k in s)
    worst = max((rel_l2(g[k], g0[k]), k) for k in g if not k.endswith("conv.bias"))
    print("\n[%s cnn=%s prec %d] full lengths vs unmasked: bitwise %s, max|dlp| %.3e, grad rel-L2 worst %.3e (%s)" % (
        cell, cnn, prec, bitwise, maxabs(lp, lp0), worst[0], worst[1]))
    assert maxabs(lp, lp0) < tol_act
    assert abs(float(loss) - float(loss0)) / abs(float(loss0)) < tol_loss
    assert worst[0] < tol_grad, worst


# ---- 6. three Adam steps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cell,cnn", [("LSTM", True), ("GRU", False)])
def test_three_adam_steps_against_packed_reference(dev, cell, cnn, prec):
    """FlatAdam on the HIP model (gradients accumulate into the flat buffer: the into_flat path of the masked BatchNorm backward) against
    torch.optim.Adam on the packed reference; the loss trajectory at the tol_loss gate of the existing three-step tests."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.optim import FlatAdam
    ops.set_precision(prec)
    tol_loss = gates(prec, 5e-5, 2e-4, 2e-5)[2]
    m, ref = build(cell, cnn, dev, reference=True)
    m.train(), ref.train()
    opt, opt_r = FlatAdam(m, lr=1e-3, weight_decay=5e-4), torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=5e-4)
    x, tg, tl = batch(LENS, max(LENS), 12, 9, m.output_lengths(LENS))
    x = fill_padding(x, LENS, "noise")
    out_len = m.output_lengths(LENS)
    losses, losses_r = [], []
    for _ in range(3):
        lp = m(x.to(dev), input_lengths=LENS)
        loss = nn.CTCLoss(reduction="sum")(lp, tg.to(dev), out_len.to(dev), tl.to(dev)) / len(LENS)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
        lp_r = ref(x, LENS)
        loss_r = tnn.CTCLoss(reduction="sum")(lp_r, tg, out_len, tl) / len(LENS)
        opt_r.zero_grad()
        loss_r.backward()
        opt_r.step()
        losses_r.append(float(loss_r))
    ops.check_health()
    print("\n[%s cnn=%s prec %d] losses %s reference %s" % (cell, cnn, prec, losses, losses_r))
    assert np.allclose(losses, losses_r, rtol=tol_loss), (losses, losses_r)


# ---- 7. the kernels through the C ABI -------------------------------------------------------------------------------
ABI_CASES = [  # layout, lens, outer, C, inner, frame
    ("rows", [50, 1, 20, 33], 200, 24, 1, 1),                 # full-length utterance, 16-B path
    ("rows", [30, 2, 11, 29], 400, 64, 1, 1),                 # T = 100: the last 280 rows (more than four 64-row tiles) are padding
    ("rows", [9, 1, 5], 27, 7, 1, 1),                         # C % 4 != 0: scalar path
    ("nchw", [25, 3, 14], 3, 5, 25 * 8, 8),                   # inner % 4 == 0
    ("nchw", [40, 1, 17, 40], 4, 3, 40 * 7, 7),               # frame 7: valid prefixes end inside a 16-B group
    ("nchw", [11, 2], 2, 4, 11 * 3, 3),                       # inner % 4 != 0: scalar path
    ("nchw", [700, 13, 350], 3, 2, 700 * 40, 40),             # planes cut into several chunks
]


@pytest.mark.parametrize("into_flat", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", ABI_CASES, ids=lambda c: "%s_%dx%dx%d" % (c[0], c[2], c[3], c[4]))
def test_masked_kernels_against_float64(dev, case, relu, into_flat):
    """ctcn_bn_fwd_train_masked / _eval_masked / ctcn_bn_bwd_masked / ctcn_mask_frames against a float64 restatement.  x, dy (and the
    buffers the outputs land in) hold NaN at every invalid element: a kernel that read one, or multiplied instead of selecting, would show
    it.  Tolerances: y, dx max-abs 2e-5 (the project's strict activation gate; the float32 expression has four roundings on values of
    magnitude <= ~10); mean / rstd / running statistics / dgamma / dbeta relative 2e-5 (float64 sums rounded once to float32, xhat in float32)."""
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    layout, lens, outer, C, inner, frame = case
    batch_n = len(lens)
    rs = np.random.RandomState(outer + C)
    v = _valid(layout, lens, outer, C, inner, frame)
    x = (2.0 * rs.standard_normal((outer, C, inner)) + 0.5).astype(np.float32)
    dy = rs.standard_normal((outer, C, inner)).astype(np.float32)
    gamma, beta = (1.0 + 0.3 * rs.standard_normal(C)).astype(np.float32), (0.2 * rs.standard_normal(C)).astype(np.float32)
    rm0, rv0 = rs.standard_normal(C).astype(np.float32), (0.5 + rs.random_sample(C)).astype(np.float32)
    eps, mom = 1e-5, 0.1
    # float64 restatement over the valid elements
    x64, dy64, n = x.astype(np.float64), dy.astype(np.float64), float(v[:, 0, :].sum())
    assert n == sum(lens) * frame
    mean = np.where(v, x64, 0).sum((0, 2)) / n
    var = np.where(v, (x64 - mean[None, :, None]) ** 2, 0).sum((0, 2)) / n
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x64 - mean[None, :, None]) * rstd[None, :, None]
    y = xh * gamma[None, :, None] + beta[None, :, None]
    keep = (y > 0) if relu else np.ones_like(v)
    y = np.where(v, np.maximum(y, 0) if relu else y, 0)
    g = np.where(v & keep, dy64, 0)
    s0, s1 = g.sum((0, 2)), np.where(v, g * xh, 0).sum((0, 2))
    dx = np.where(v, gamma[None, :, None] * rstd[None, :, None] * (g - s0[None, :, None] / n - xh * s1[None, :, None] / n), 0)
    y_eval = (x64 - rm0[None, :, None]) / np.sqrt(rv0 + eps)[None, :, None] * gamma[None, :, None] + beta[None, :, None]
    y_eval = np.where(v, np.maximum(y_eval, 0) if relu else y_eval, 0)

    def poisoned(a):
        return torch.from_numpy(np.where(v, a, np.nan).astype(np.float32)).to(dev)

    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    xd, dyd = poisoned(x), poisoned(dy)
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    rm, rv = torch.from_numpy(rm0).to(dev), torch.from_numpy(rv0).to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    yd = torch.full_like(xd, float("nan"))
    sm, sr = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(int(L.ctcn_bn_masked_ws_bytes(outer, C, inner)), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    geom = (batch_n if layout == "rows" else outer, frame, outer, C, inner)
    _lib.check(L.ctcn_bn_fwd_train_masked(P(xd), P(yd), P(gd), P(bd), P(rm), P(rv), P(sm), P(sr), P(lens_d), *geom, eps, mom, relu, P(ws), ws.numel(),
                                          st, P(nbt)), "fwd")
    assert int(nbt) == 1
    rel = lambda a, b: float(np.max(np.abs(a.cpu().numpy().astype(np.float64) - b) / np.maximum(np.abs(b), 1e-3)))
    assert rel(sm, mean) < 2e-5 and rel(sr, rstd) < 2e-5
    assert rel(rm, (1 - mom) * rm0 + mom * mean) < 2e-5 and rel(rv, (1 - mom) * rv0 + mom * var * n / (n - 1)) < 2e-5
    got = yd.cpu().numpy()
    assert np.isfinite(got).all() and np.all(got[~v] == 0)
    assert np.max(np.abs(got - y)) < 2e-5
    # the same input bits give the same output bits
    yd2, rm2, rv2 = torch.full_like(xd, float("nan")), torch.from_numpy(rm0).to(dev), torch.from_numpy(rv0).to(dev)
    sm2, sr2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
    _lib.check(L.ctcn_bn_fwd_train_masked(P(xd), P(yd2), P(gd), P(bd), P(rm2), P(rv2), P(sm2), P(sr2), P(lens_d), *geom, eps, mom, relu, P(ws),
                                          ws.numel(), st, None), "fwd again")
    assert torch.equal(yd2, yd) and torch.equal(sm2, sm) and torch.equal(sr2, sr) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
    # backward; into_flat: dgamma / dbeta accumulate (beta_acc = 1) into what the buffers hold
    base_g, base_b = rs.standard_normal(C).astype(np.float32), rs.standard_normal(C).astype(np.float32)
    dg, db = torch.from_numpy(base_g.copy()).to(dev), torch.from_numpy(base_b.copy()).to(dev)
    dxd = torch.full_like(xd, float("nan"))
    _lib.check(L.ctcn_bn_bwd_masked(P(xd), P(yd) if relu else None, P(dyd), P(gd), P(sm), P(sr), P(dxd), P(dg), P(db), P(lens_d), *geom, relu,
                                    1.0 if into_flat else 0.0, P(ws), ws.numel(), st), "bwd")
    got = dxd.cpu().numpy()
    assert np.isfinite(got).all() and np.all(got[~v] == 0)
    assert np.max(np.abs(got - dx)) < 2e-5 * max(1.0, float(np.abs(dx).max()))
    scale = max(1.0, float(np.abs(s1).max()), float(np.abs(s0).max()))
    add_g, add_b = (base_g, base_b) if into_flat else (0.0, 0.0)
    assert np.max(np.abs(dg.cpu().numpy() - (s1 + add_g))) < 2e-5 * scale and np.max(np.abs(db.cpu().numpy() - (s0 + add_b))) < 2e-5 * scale
    # eval forward and the mask op (out of place, then in place)
    ye = torch.full_like(xd, float("nan"))
    rm_e, rv_e = torch.from_numpy(rm0).to(dev), torch.from_numpy(rv0).to(dev)
    _lib.check(L.ctcn_bn_fwd_eval_masked(P(xd), P(ye), P(gd), P(bd), P(rm_e), P(rv_e), P(lens_d), *geom, eps, relu, st), "eval")
    got = ye.cpu().numpy()
    assert np.isfinite(got).all() and np.all(got[~v] == 0) and np.max(np.abs(got - y_eval)) < 2e-5 * max(1.0, float(np.abs(y_eval).max()))
    ym = torch.full_like(xd, float("nan"))
    _lib.check(L.ctcn_mask_frames(P(xd), P(ym), P(lens_d), *geom, st), "mask")
    want = np.where(v, x, 0).astype(np.float32)
    assert np.array_equal(ym.cpu().numpy(), want)
    _lib.check(L.ctcn_mask_frames(P(xd), P(xd), P(lens_d), *geom, st), "mask in place")
    assert np.array_equal(xd.cpu().numpy(), want)


FULL_LENGTH_CASES = [  # layout, outer, C, inner, batch, frame, storage offset of x (floats), option bn_rows4
    ("rows", 200, 24, 1, 4, 1, 0, 1),                         # 16-B path
    ("rows", 400, 64, 1, 4, 1, 0, 1),
    ("rows", 27, 7, 1, 3, 1, 0, 1),                           # C % 4 != 0: scalar path
    ("rows", 1500, 64, 1, 4, 1, 1, 1),                        # x 4-B aligned only: the dword kernels although C % 4 == 0
    ("rows", 400, 64, 1, 4, 1, 0, 0),                         # the dword reductions by option
    ("nchw", 3, 5, 200, 3, 8, 0, 1),                          # inner % 4 == 0: vector path
    ("nchw", 2, 4, 33, 2, 3, 0, 1),                           # scalar path
    ("nchw", 3, 2, 28000, 3, 40, 0, 1),                       # planes cut into several chunks (ich > 1)
    ("nchw", 200, 64, 37, 200, 1, 0, 1),                      # several planes per chunk (opc > 1)
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", FULL_LENGTH_CASES, ids=lambda c: "%s_%dx%dx%d_off%d_rows4_%d" % (c[0], c[1], c[2], c[3], c[6], c[7]))
def test_full_length_masked_kernels_equal_dense_bit_for_bit(dev, case, relu):
    """With lens = [tmax] * batch the length-aware entry points sum the same values in the same order as the dense ones and evaluate the
    same per-element expressions: ctcn_bn_fwd_train / _masked, ctcn_bn_bwd / _masked and ctcn_bn_fwd_eval / _masked agree bit for bit
    (the counts are the same doubles, 1 / n the same correctly rounded division)."""
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    layout, outer, C, inner, batch_n, frame, xoff, rows4 = case
    tmax = outer // batch_n if layout == "rows" else inner // frame
    rs = np.random.RandomState(outer + C + inner)
    shape = (outer, C, inner)
    buf = torch.empty(outer * C * inner + xoff, device=dev)
    xd = buf[xoff:].view(shape)
    xd.copy_(torch.from_numpy((2.0 * rs.standard_normal(shape) + 0.5).astype(np.float32)))
    assert xd.data_ptr() % 16 == 4 * xoff
    dyd = torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dev)
    gd = torch.from_numpy((1.0 + 0.3 * rs.standard_normal(C)).astype(np.float32)).to(dev)
    bd = torch.from_numpy((0.2 * rs.standard_normal(C)).astype(np.float32)).to(dev)
    rm0, rv0 = torch.from_numpy(rs.standard_normal(C).astype(np.float32)).to(dev), torch.from_numpy((0.5 + rs.random_sample(C)).astype(np.float32)).to(dev)
    lens_d = torch.tensor([tmax] * batch_n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.ctcn_bn_masked_ws_bytes(outer, C, inner)), dtype=torch.uint8, device=dev)
    assert ws.numel() >= int(L.ctcn_bn_ws_bytes(outer, C, inner)) > 0
    st, eps, mom = _lib.stream_ptr(), 1e-5, 0.1
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    nan = lambda *s: torch.full(s, float("nan"), device=dev)

    def run(masked):
        geom = (P(lens_d), batch_n, frame) if masked else ()
        sfx = "_masked" if masked else ""
        o = {"y": nan(*shape), "save_mean": nan(C), "save_rstd": nan(C), "running_mean": rm0.clone(), "running_var": rv0.clone(),
             "dx": nan(*shape), "dgamma": nan(C), "dbeta": nan(C), "eval_y": nan(*shape)}
        _lib.check(getattr(L, "ctcn_bn_fwd_train" + sfx)(P(xd), P(o["y"]), P(gd), P(bd), P(o["running_mean"]), P(o["running_var"]), P(o["save_mean"]),
                                                         P(o["save_rstd"]), *geom, outer, C, inner, eps, mom, relu, P(ws), ws.numel(), st, None), "fwd" + sfx)
        _lib.check(getattr(L, "ctcn_bn_bwd" + sfx)(P(xd), P(o["y"]) if relu else None, P(dyd), P(gd), P(o["save_mean"]), P(o["save_rstd"]), P(o["dx"]),
                                                   P(o["dgamma"]), P(o["dbeta"]), *geom, outer, C, inner, relu, 0.0, P(ws), ws.numel(), st), "bwd" + sfx)
        _lib.check(getattr(L, "ctcn_bn_fwd_eval" + sfx)(P(xd), P(o["eval_y"]), P(gd), P(bd), P(rm0), P(rv0), *geom, outer, C, inner, eps, relu, st), "eval" + sfx)
        torch.cuda.synchronize()
        return o

    before = L.ctcn_get_option(b"bn_rows4")
    try:
        _lib.check(L.ctcn_set_option(b"bn_rows4", rows4), "set_option")
        dense, masked = run(False), run(True)
    finally:
        L.ctcn_set_option(b"bn_rows4", before)
    for k in dense:
        assert bool(torch.isfinite(dense[k]).all()), k
        assert torch.equal(masked[k], dense[k]), (k, maxabs(masked[k], dense[k]))


def test_mask_frames_autograd_and_layouts(dev):
    from ctc_pytorch_amd import ops
    lens = [5, 1, 3]
    for layout, shape, taxis, baxis in (("tbc", (5, 3, 8), 0, 1), ("btf", (3, 5, 6), 1, 0), ("bctf", (3, 2, 5, 6), 2, 0)):
        x = torch.randn(*shape, device=dev, requires_grad=True)
        y = ops.mask_frames(x, torch.tensor(lens), layout)
        y.backward(torch.ones_like(y))
        idx = [None] * len(shape)
        t = torch.arange(shape[taxis], device=dev)
        view_t, view_b = [1] * len(shape), [1] * len(shape)
        view_t[taxis], view_b[baxis] = shape[taxis], shape[baxis]
        m = t.view(view_t) < torch.tensor(lens, device=dev).view(view_b)
        assert torch.equal(y.detach(), torch.where(m, x.detach(), torch.zeros((), device=dev))) and torch.equal(x.grad, m.expand(shape).float())
    # lengths already on the device are taken as they are
    y = ops.mask_frames(torch.ones(5, 3, 4, device=dev), torch.tensor(lens, device=dev), "tbc")
    assert y.sum().item() == 4 * sum(lens)


# ---- 8. synchronised BatchNorm --------------------------------------------------------------------------------------
def test_sync_bn_with_lengths_raises(dev):
    from ctc_pytorch_amd import ops
    m, _ = build("LSTM", False, dev)
    m.train()
    x, _, _ = batch(LENS, max(LENS), 12, 9, LENS)
    ops.set_sync_bn(lambda sums, n: n)
    try:
        with pytest.raises(NotImplementedError, match="ynchronised BatchNorm"):
            m(x.to(dev), input_lengths=LENS)
    finally:
        ops.set_sync_bn(None)
    torch.cuda.synchronize()


# ---- the decode driver ----------------------------------------------------------------------------------------------
def test_decode_driver_strings_do_not_depend_on_the_batch(dev):
    """steps/decode_ctc.decode_and_score(mask_padding=True) over one ragged minibatch gives the error rates of the same utterances decoded
    one per minibatch (greedy decoder); the decoder sees model.output_lengths(...) frames."""
    from ctc_pytorch_amd.steps import decode_ctc
    from ctc_pytorch_amd.utils.ctcDecoder import GreedyDecoder
    V, T = 9, max(LENS)
    m, _ = build("LSTM", True, dev)
    x, tg, tl = batch(LENS, T, 12, V, m.output_lengths(LENS))
    frac = torch.tensor([np.float32(float(l) / float(T)) for l in LENS])
    words = synth.int2char(V)
    together = [(x, frac, tg, tl, ["u%d" % b for b in range(len(LENS))])]
    alone = [(x[b:b + 1, :l].contiguous(), torch.ones(1), tg[b:b + 1], tl[b:b + 1], ["u%d" % b]) for b, l in enumerate(LENS)]
    seen = []

    class Recording(GreedyDecoder):
        def decode(self, probs, lens):
            out = super().decode(probs, lens)
            seen.append((list(lens), out))
            return out

    runs = []
    for data in (together, alone):
        del seen[:]
        dec = Recording(words, space_idx=-1, blank_index=0)
        rates = decode_ctc.decode_and_score(m, data, dec, words, dev, log=lambda *_: None, mask_padding=True)
        runs.append((rates, [n for lens, _ in seen for n in lens], [s for _, out in seen for s in out]))
    assert runs[0][1] == m.output_lengths(LENS).tolist() == runs[1][1]
    assert runs[0][2] == runs[1][2] and runs[0][0] == runs[1][0]
