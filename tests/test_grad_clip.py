"""Gradient-norm clipping and the non-finite-step guard on the HIP kernels (ctcn_grad_norm, ctcn_clip_control, ctcn_adam_step_ex,
ctcn_scale_by_device_scalar through ops / optim.FlatAdam / nn.utils) against the float64 restatement of tests/test_grad_clip_host.py.

Bounds: the norm is a double sum of exact squares (relative error ~1e-16), so it must equal the float32 rounding of numpy's float64 value
to within ONE float32 ulp (the final rounding); the infinity norm is exact; a fused step that does not clip equals the plain fused Adam bit
for bit; a clipping step is held to test_adam_vs_oracle's own bound (max-abs 2e-6) -- the extra error is one float32 multiply per element."""
import copy

import numpy as np
import pytest
import torch

from ctc_pytorch_amd.testing import synth
from test_grad_clip_host import clip_then_adam_ref, total_norm_ref

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _bits(t):
    return int(t.detach().reshape(1).view(torch.int32).item())


def _ulps(a, b):
    """Distance in float32 ulps of two non-negative finite float32 values."""
    ia, ib = int(np.float32(a).view(np.int32)), int(np.float32(b).view(np.int32))
    return abs(ia - ib)


def _data(kind, n, seed=0):
    rs = np.random.RandomState(seed + n % 1000)
    g = rs.standard_normal(n).astype(np.float32)
    if kind == "zero":
        g[:] = 0
    elif kind == "huge":
        g[n // 2] = np.float32(1e30)                       # its square overflows float32, not double
    elif kind == "denormal":
        g = (rs.standard_normal(n) * 1e-42).astype(np.float32)
        assert n < 3 or np.any((g != 0) & (np.abs(g) < np.finfo(np.float32).tiny))
    return g


def _check_norms(dev, t, g, offsets):
    """t: device buffer holding g.  Total and per-segment L2 norms within 1 ulp of the float64 value, infinity norms exact."""
    from ctc_pytorch_amd import ops
    for nt in (2.0, INF):
        total, segs = ops.grad_norm(t, nt, segments=offsets)
        alone = ops.grad_norm(t, nt)
        assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
        got, seg_got = float(total.item()), segs.cpu().numpy()
        assert _bits(alone) == _bits(total)
        want = np.float32(total_norm_ref(g, nt))
        if nt == INF:
            assert np.float32(got) == want, (got, want)
        else:
            assert np.isfinite(got) and _ulps(got, want) <= 1, (got, want)
        for s, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            w = np.float32(total_norm_ref(g[lo:hi], nt)) if hi > lo else np.float32(0)
            if nt == INF:
                assert seg_got[s] == w, (s, seg_got[s], w)
            else:
                assert _ulps(seg_got[s], w) <= 1, (s, seg_got[s], w)


# ---------------------------------------------------------------------------------------------------------
# 1. norm value
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "zero", "huge", "denormal"])
@pytest.mark.parametrize("n", [1, 3, 255, 10007])
def test_norm_value(dev, n, kind):
    g = _data(kind, n)
    offsets = [0, n] if n < 3 else [0, n // 3, n // 3, n - 1, n]           # an empty segment and a one-element one among them
    _check_norms(dev, torch.from_numpy(g).to(dev), g, offsets)


@pytest.mark.parametrize("kind", ["gauss", "zero", "huge", "denormal"])
def test_norm_value_misaligned_slice(dev, kind):
    """n not a multiple of 4, two chunks, starting 12 bytes into an allocation: the dword path of the same element -> lane map."""
    n = 20483
    g = _data(kind, n)
    big = torch.full((n + 64,), 7.0, device=dev)                            # the neighbours must not leak into the result
    big[3:3 + n].copy_(torch.from_numpy(g))
    t = big[3:3 + n]
    assert t.data_ptr() % 16 == 12
    _check_norms(dev, t, g, [0, 5, 16384, 16385, n])


@pytest.fixture(scope="module")
def cfg2_opt(dev):
    """The flat gradient buffer of a cfg2-shaped model (4 x 320 BiLSTM, 62 classes: 8.3 M elements, 509 chunks) and its per-tensor offsets."""
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.optim import FlatAdam
    rp = {"rnn_input_size": 40, "rnn_hidden_size": 320, "rnn_layers": 4, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    torch.manual_seed(2)
    opt = FlatAdam(CTC_Model(rnn_param=rp, num_class=62, drop_out=0.1).to(dev))
    offs = sorted(off for _, off, _, _ in opt._slices()) + [opt.grad.numel()]
    return opt, offs


@pytest.mark.parametrize("kind", ["gauss", "zero", "huge", "denormal"])
def test_norm_value_cfg2_flat_gradient(dev, cfg2_opt, kind):
    opt, offs = cfg2_opt
    n = opt.grad.numel()
    assert n > 8_000_000 and len(offs) > 20
    g = _data(kind, n)
    opt.grad.copy_(torch.from_numpy(g))
    _check_norms(dev, opt.grad, g, offs)
    opt.grad.zero_()


def test_nonfinite_values_reach_the_norm_as_in_torch(dev):
    from ctc_pytorch_amd import ops
    n = 40000
    base = _data("gauss", n)
    for bad, pos in (([np.nan], [17]), ([np.inf], [n - 1]), ([-np.inf], [20000]), ([np.inf, np.nan], [3, 39000]), ([np.nan, np.inf], [3, 39000])):
        g = base.copy()
        g[pos] = bad
        t = torch.from_numpy(g).to(dev)
        for nt in (2.0, INF):
            ctl = ops.new_clip_ctl(dev)
            got = float(ops.grad_norm(t, nt, ctl=ctl).item())
            want = float(torch.linalg.vector_norm(torch.from_numpy(g), nt))
            assert (np.isnan(got) and np.isnan(want)) or got == want, (bad, nt, got, want)
            assert int(ctl[ops.CTL_NONFINITE].item()) == 1
    ctl = ops.new_clip_ctl(dev)
    ops.grad_norm(torch.from_numpy(base).to(dev), 2.0, ctl=ctl)
    assert int(ctl[ops.CTL_NONFINITE].item()) == 0
    # a float32 norm that overflows although every element is finite counts as non-finite (torch's own float32 norm is inf there too)
    ops.grad_norm(torch.full((8,), 3e38, device=dev), 2.0, ctl=ctl)
    assert int(ctl[ops.CTL_NONFINITE].item()) == 1 and float(ctl.view(torch.float32)[ops.CTL_NORM].item()) == INF


# ---------------------------------------------------------------------------------------------------------
# 2. determinism
# ---------------------------------------------------------------------------------------------------------
def test_norm_is_a_function_of_the_bits_alone(dev):
    """Same values -> same bits: across 20 calls, across grids forced through the ABI's `grid_blocks` argument (1, 7, 64, 1000 workgroups
    against the default sized from ctcn_device_cus()), on a second stream, from a differently aligned copy, and with zeros appended
    (a sub-range of a padded buffer against the whole of it)."""
    from ctc_pytorch_amd import ops
    n = 1_000_003
    g = _data("gauss", n, seed=5)
    t = torch.from_numpy(g).to(dev)
    for nt in (2.0, INF):
        ref = _bits(ops.grad_norm(t, nt))
        assert all(_bits(ops.grad_norm(t, nt)) == ref for _ in range(20))
        for blocks in (1, 7, 64, 1000):
            assert _bits(ops.grad_norm(t, nt, blocks=blocks)) == ref, blocks
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            on_side = [ops.grad_norm(t, nt) for _ in range(3)]
        side.synchronize()
        assert all(_bits(x) == ref for x in on_side)
        padded = torch.zeros(n + 50_001, device=dev)
        padded[:n].copy_(t)
        assert _bits(ops.grad_norm(padded[:n], nt)) == ref and _bits(ops.grad_norm(padded, nt)) == ref
        shifted = torch.zeros(n + 8, device=dev)
        shifted[1:1 + n].copy_(t)
        assert shifted[1:].data_ptr() % 16 == 4 and _bits(ops.grad_norm(shifted[1:1 + n], nt)) == ref
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# twins of the small model the other suites train (2 x 16 BiLSTM)
# ---------------------------------------------------------------------------------------------------------
RP = {"rnn_input_size": 40, "rnn_hidden_size": 16, "rnn_layers": 2, "bidirectional": True, "batch_norm": True}


def _twins(dev, k, seed=3, V=12):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    torch.manual_seed(seed)
    m = CTC_Model(rnn_param=dict(RP, rnn_type=nn.LSTM), num_class=V, drop_out=0.0)
    return [copy.deepcopy(m).to(dev) for _ in range(k)]


def _fake_grads(model, k, seed=5, scale=1.0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [[torch.randn(p.shape, generator=gen) * scale for p in model.parameters()] for _ in range(k)]


def _set_grads(opt, model, gs):
    opt.zero_grad()
    for p, g in zip(model.parameters(), gs):
        p.grad.copy_(g.to(p.device))


def _same_state(a, b):
    return torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


# ---------------------------------------------------------------------------------------------------------
# 3. the fused step that does not clip is today's step
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["inf", "10x", "guard_only", "10x_inf_norm_guard"])
def test_fused_step_without_clipping_equals_plain_step(dev, case):
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.optim import FlatAdam
    m_off, m_on = _twins(dev, 2)
    grads = _fake_grads(m_off, 3)
    flat_norms = [total_norm_ref(np.concatenate([g.numpy().ravel() for g in gs])) for gs in grads]
    kw = {"inf": dict(max_grad_norm=INF), "10x": dict(max_grad_norm=10 * max(flat_norms)), "guard_only": dict(skip_nonfinite=True),
          "10x_inf_norm_guard": dict(max_grad_norm=10 * max(flat_norms), norm_type=INF, skip_nonfinite=True)}[case]
    off = FlatAdam(m_off, lr=2e-3, weight_decay=5e-4)
    on = FlatAdam(m_on, lr=2e-3, weight_decay=5e-4, **kw)
    assert on.last_grad_norm is None and on.skipped_steps == 0
    for k, gs in enumerate(grads):
        _set_grads(off, m_off, gs)
        _set_grads(on, m_on, gs)
        before = on.grad.clone()
        off.step()
        on.step()
        assert _same_state(off, on), (case, k)
        assert torch.equal(on.grad, before)                                 # the fused path does not write the gradient back
        if kw.get("norm_type", 2.0) == 2.0:
            assert _ulps(float(on.last_grad_norm.item()), np.float32(flat_norms[k])) <= 1
    assert on.step_count == off.step_count == 3 and on.skipped_steps == 0
    assert float(on._ctl.view(torch.float32)[ops.CTL_COEF].item()) == 1.0
    for a, b in zip(m_off.parameters(), m_on.parameters()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------
# 4. the fused step that clips, against the yardstick
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type,max_norm", [(2.0, 10.0), (INF, 0.4)])
def test_fused_clipped_adam_vs_restatement(dev, norm_type, max_norm):
    """test_adam_vs_oracle's data (n = 10 007, gradients g * step, lr 1e-3, wd 5e-4) with a max_norm that makes the coefficient ~0.1
    (|g| ~ 100, 200, 300; max |g| ~ 4, 8, 12), at that test's bound."""
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(4)
    n = 10007
    p, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    m, v, pr = np.zeros(n), np.zeros(n), p.astype(np.float64)
    pt, mt, vt = torch.from_numpy(p).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ctl = ops.new_clip_ctl(dev)
    for step in range(1, 4):
        gs = (g * step).astype(np.float32)
        pr, m, v, norm, coef = clip_then_adam_ref(pr, gs, m, v, step, 1e-3, 5e-4, max_norm, norm_type)
        gt = torch.from_numpy(gs).to(dev)
        ops.grad_norm(gt, norm_type, ctl=ctl)
        ops.clip_control(ctl, max_norm, 1e-3, 0.9, 0.999, False)
        ops.adam_step_ex(pt, gt, mt, vt, 0.9, 0.999, 1e-8, 5e-4, ctl)
        f = ctl.view(torch.float32)
        assert 0.02 < coef < 0.12 and abs(float(f[ops.CTL_COEF].item()) - coef) < 3e-7 * coef          # two float32 roundings (norm, quotient)
        assert int(ctl[ops.CTL_STEP].item()) == step and int(ctl[ops.CTL_APPLY].item()) == 1
        # ctcn_adam_step's host expressions on the float32 arguments, evaluated on the device: at most the rounding of pow() apart
        lr32, b1, b2 = np.float64(np.float32(1e-3)), np.float64(np.float32(0.9)), np.float64(np.float32(0.999))
        assert _ulps(float(f[ops.CTL_STEP_SIZE].item()), np.float32(lr32 / (1 - b1 ** step))) <= 1
        assert _ulps(float(f[ops.CTL_SQRT_BC2].item()), np.float32(np.sqrt(1 - b2 ** step))) <= 1
    err = float(np.max(np.abs(pt.cpu().numpy().astype(np.float64) - pr)))
    print("clipped adam vs restatement: max-abs %.3e (norm_type %s)" % (err, norm_type))
    assert err < 2e-6
    assert float(np.max(np.abs(mt.cpu().numpy().astype(np.float64) - m))) < 2e-6


# ---------------------------------------------------------------------------------------------------------
# 5. the stand-alone clip
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_clip_grad_norm_scales_in_place(dev, norm_type):
    from ctc_pytorch_amd import ops
    n = 10007
    g = _data("gauss", n, seed=9)
    t = torch.from_numpy(g).to(dev)
    before = t.clone()
    ctl = ops.new_clip_ctl(dev)
    max_norm = 3.0 if norm_type == 2.0 else 0.25
    total = ops.clip_grad_norm_(t, max_norm, norm_type, ctl=ctl)
    coef = ctl.view(torch.float32)[ops.CTL_COEF].clone()
    tn = np.float32(total.item())
    assert _ulps(tn, np.float32(total_norm_ref(g, norm_type))) <= (1 if norm_type == 2.0 else 0)          # the PRE-clip norm
    assert np.float32(coef.item()) == np.float32(max_norm) / (tn + np.float32(1e-6)) and coef.item() < 0.1  # torch's expression, in float32
    assert torch.equal(t.view(torch.int32), (before * coef).view(torch.int32))
    # below the threshold the coefficient clamps to 1 and nothing moves
    again = t.clone()
    total2 = ops.clip_grad_norm_(t, 1e6, norm_type, ctl=ctl)
    assert float(ctl.view(torch.float32)[ops.CTL_COEF].item()) == 1.0 and torch.equal(t, again)
    assert float(total2.item()) <= max_norm * (1 + 1e-6)
    # a non-finite norm: error_if_nonfinite raises and leaves the gradient alone; without it the NaN coefficient poisons every element (torch)
    t[5] = float("nan")
    keep = t.clone()
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.clip_grad_norm_(t, 1.0, norm_type, error_if_nonfinite=True)
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32))
    assert torch.isnan(ops.clip_grad_norm_(t, 1.0, norm_type)) and bool(torch.isnan(t).all())
    with pytest.raises(ValueError):
        ops.clip_grad_norm_(t, 0.0)


def test_nn_utils_clip_equals_optimizer_clip(dev):
    """The reference's commented-out line, un-commented: nn.utils.clip_grad_norm_(model.parameters(), c) on a FlatAdam-homed CTC_Model runs
    on the flat buffer and gives the bits of optimizer.clip_grad_norm_(c); a subset of the parameters is torch's business."""
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.optim import FlatAdam
    m1, m2, m3 = _twins(dev, 3)
    o1, o2, o3 = FlatAdam(m1), FlatAdam(m2), FlatAdam(m3)
    gs = _fake_grads(m1, 1)[0]
    for o, m in ((o1, m1), (o2, m2), (o3, m3)):
        _set_grads(o, m, gs)
    assert nn._flat_grad_of(list(m1.parameters())).data_ptr() == o1.grad.data_ptr()
    c = 0.5
    before = o1.grad.clone()
    n1 = nn.utils.clip_grad_norm_(m1.parameters(), c)
    n2 = o2.clip_grad_norm_(c)
    assert n1.is_cuda and _bits(n1) == _bits(n2) and torch.equal(o1.grad.view(torch.int32), o2.grad.view(torch.int32))
    assert not torch.equal(o1.grad, before) and all(torch.equal(p.grad, p._ctcn_grad) for p in m1.parameters())
    want = total_norm_ref(before.cpu().numpy())
    assert _ulps(float(n1.item()), np.float32(want)) <= 1
    assert abs(total_norm_ref(o1.grad.cpu().numpy()) - c) < 1e-5
    # a subset does not cover the buffer: torch's kernels on the views (same mathematics, its own summation order)
    sub = list(m3.parameters())[:3]
    n3 = nn.utils.clip_grad_norm_(sub, 1e-3)
    ref = total_norm_ref(np.concatenate([g.numpy().ravel() for g in gs[:3]]))
    assert abs(float(n3.item()) - ref) < 1e-5 * ref


# ---------------------------------------------------------------------------------------------------------
# 6. the guard
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 1.0])
def test_guard_drops_nonfinite_steps_and_keeps_the_step_count(dev, clip):
    from ctc_pytorch_amd.optim import FlatAdam
    ma, mb, mc, md = _twins(dev, 4)
    kw = dict(lr=2e-3, weight_decay=5e-4, max_grad_norm=clip, skip_nonfinite=True)
    a, b, c = FlatAdam(ma, **kw), FlatAdam(mb, **kw), FlatAdam(mc, **kw)
    g1, g2, g3 = _fake_grads(ma, 3)
    for o, m in ((a, ma), (b, mb)):
        _set_grads(o, m, g1)
        o.step()
    assert _same_state(a, b) and a.skipped_steps == 0 and a.step_count == 1
    held = [t.clone() for t in (a.flat, a.m, a.v)]
    for k, bad in enumerate((float("nan"), INF), 1):
        _set_grads(a, ma, g2)
        a.grad[a.grad.numel() // 2] = bad
        a.step()
        assert all(torch.equal(x, y) for x, y in zip(held, (a.flat, a.m, a.v))), bad
        assert a.skipped_steps == k and a.step_count == 1
        assert not np.isfinite(float(a.last_grad_norm.item()))
    # the next finite step is the step of a twin that never saw the bad gradients: the bias-correction count did not advance
    for o, m in ((a, ma), (b, mb)):
        _set_grads(o, m, g2)
        o.step()
    assert _same_state(a, b) and a.step_count == b.step_count == 2 and a.skipped_steps == 2 and b.skipped_steps == 0
    sd = copy.deepcopy(a.state_dict())
    assert all(float(st["step"]) == 2.0 for st in sd["state"].values()) and len(sd["state"]) == len(list(ma.parameters()))
    # the torch-Adam layout is unchanged: the package loads into torch.optim.Adam with the right step
    ta = torch.optim.Adam(md.parameters(), lr=2e-3, weight_decay=5e-4)
    ta.load_state_dict(sd)
    assert all(float(st["step"]) == 2.0 for st in ta.state.values())
    # load_state_dict (the driver's rollback) restores the device step counter: after a round trip the third step is the twin's
    c.load_state_dict(sd)
    c.flat.copy_(a.flat)
    assert c.step_count == 2
    a.load_state_dict({"state": {}, "param_groups": sd["param_groups"]})     # a fresh optimiser's package ...
    assert a.step_count == 0 and float(a.m.abs().max()) == 0.0
    a.load_state_dict(sd)                                                     # ... and back
    for o, m in ((a, ma), (b, mb), (c, mc)):
        _set_grads(o, m, g3)
        o.step()
    assert _same_state(a, b) and _same_state(c, b) and a.step_count == b.step_count == c.step_count == 3


def test_without_the_guard_a_nonfinite_gradient_poisons_the_parameters(dev):
    """The default (skip_nonfinite=False) with clipping on is torch's behaviour: clip_grad_norm_ scales by a NaN coefficient, Adam writes NaN."""
    from ctc_pytorch_amd.optim import FlatAdam
    (m,) = _twins(dev, 1)
    o = FlatAdam(m, lr=2e-3, weight_decay=5e-4, max_grad_norm=1.0)
    _set_grads(o, m, _fake_grads(m, 1)[0])
    o.grad[7] = float("nan")
    o.step()
    assert bool(torch.isnan(o.flat).all()) and bool(torch.isnan(o.m).all()) and o.step_count == 1 and o.skipped_steps == 0


def test_switching_the_features_on_a_live_optimizer_keeps_the_step_count(dev):
    """max_grad_norm / skip_nonfinite are plain attributes: guarded steps, then plain steps, then guarded ones again, with a dropped step
    in between, count as a twin counts that took the same applied steps with the features off throughout; and last_grad_norm follows
    the explicit clip_grad_norm_() as well as step()."""
    from ctc_pytorch_amd.optim import FlatAdam
    ma, mb = _twins(dev, 2)
    a, b = FlatAdam(ma, lr=2e-3, weight_decay=5e-4, skip_nonfinite=True), FlatAdam(mb, lr=2e-3, weight_decay=5e-4)
    grads = _fake_grads(ma, 5)
    plan = [(True, False), (True, True), (False, False), (False, False), (True, False), (True, False)]        # (guard on, bad gradient)
    k = 0
    for guard, bad in plan:
        a.skip_nonfinite = guard
        _set_grads(a, ma, grads[k])
        if bad:
            a.grad[3] = float("nan")
            a.step()
            continue
        _set_grads(b, mb, grads[k])
        a.step()
        b.step()
        k += 1
        assert _same_state(a, b), k
    assert a.step_count == b.step_count == 5 and a.skipped_steps == 1
    assert float(a.state_dict()["state"][0]["step"]) == 5.0
    _set_grads(a, ma, grads[0])
    want = np.float32(total_norm_ref(a.grad.cpu().numpy()))
    total = a.clip_grad_norm_(0.5)
    assert _bits(total) == _bits(a.last_grad_norm) and _ulps(float(total.item()), want) <= 1
    assert a.step_count == 5                                                # the explicit clip has a control block of its own
    a.step()
    assert a.step_count == 6 and abs(float(a.last_grad_norm.item()) - 0.5) < 1e-5


# ---------------------------------------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_training_steps_clip_and_survive_an_infeasible_utterance(dev, prec):
    """Three training steps of the small model with every step clipped; on step 2 one utterance has more labels than frames, so with
    zero_infinity=False its loss is +inf and its gradient rows NaN: the guard drops that step (parameters bit-identical), steps 1 and 3
    move them and the loss of step 3 is finite.  Run with the weight-gradient side stream forced on and with it off: same bits."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.optim import FlatAdam
    ops.set_precision(prec)
    V, B, T = 12, 4, 30
    b = synth.make_batch(seed=3, B=B, T=T, F=40, V=V, lab_lo=3, lab_hi=6)
    x = torch.from_numpy(b["x"]).to(dev)
    tg, tl = torch.from_numpy(b["targets"]).to(dev), torch.from_numpy(b["tgt_len"]).to(dev)
    loss_fn = nn.CTCLoss(reduction="sum", zero_infinity=False)
    max_norm = 0.05
    old = (ops._side["enabled"], ops._side["min_items"], ops._side["min_items_bwd"])

    def run(side):
        ops.set_side_stream(side, 0)
        (model,) = _twins(dev, 1, V=V)
        model.train()
        opt = FlatAdam(model, lr=1e-2, weight_decay=5e-4, max_grad_norm=max_norm, skip_nonfinite=True)
        flats, losses, norms = [opt.flat.clone()], [], []
        for step in (1, 2, 3):
            out = model(x)
            in_len = torch.full((B,), out.size(0), dtype=torch.int64)
            if step == 2:
                in_len[0] = int(b["tgt_len"][0]) - 1                          # fewer frames than labels: infeasible
            loss = loss_fn(out, tg, in_len.to(dev), tl) / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            flats.append(opt.flat.clone())
            losses.append(float(loss.item()))
            norms.append(float(opt.last_grad_norm.item()))
        torch.cuda.synchronize()
        ops.check_health(dev)
        return flats, losses, norms, opt.skipped_steps, opt.step_count

    try:
        flats, losses, norms, skipped, steps = run(True)
        flats_off, losses_off, norms_off, _, _ = run(False)
    finally:
        ops.set_side_stream(*old)
    assert not torch.equal(flats[1], flats[0]) and torch.equal(flats[2], flats[1]) and not torch.equal(flats[3], flats[2])
    assert all(bool(torch.isfinite(f).all()) for f in flats)
    assert losses[1] == INF and np.isfinite(losses[0]) and np.isfinite(losses[2])
    assert norms[0] > max_norm and norms[2] > max_norm and not np.isfinite(norms[1])          # every applied step was clipped
    assert (skipped, steps) == (1, 2)
    assert all(torch.equal(p, q) for p, q in zip(flats, flats_off)) and losses == losses_off and norms[0] == norms_off[0] and norms[2] == norms_off[2]
