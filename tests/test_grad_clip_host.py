"""Gradient-norm clipping and the non-finite-step guard, the part that runs without a GPU: the float64 numpy restatement of
"clip_grad_norm_, then Adam" that tests/test_grad_clip.py holds the fused kernels to (pinned here against torch's own two calls on CPU
tensors), the `nn.utils` namespace, the place of the clipped step in run_epoch, the driver options and FlatAdam's argument checks."""
import numpy as np
import pytest
import torch

from oracle import np_ref as R


# ---------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------
def total_norm_ref(g, norm_type=2.0):
    g = np.asarray(g, dtype=np.float64)
    return float(np.max(np.abs(g))) if norm_type == float("inf") else float(np.sqrt(np.sum(g * g)))


def clip_coef_ref(norm, max_norm):
    """torch's expression: clamp(max_norm / (total_norm + 1e-6), max=1)."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def clip_then_adam_ref(p, g, m, v, step, lr, wd, max_norm, norm_type=2.0):
    """One step of clip_grad_norm_(max_norm) followed by Adam (L2-coupled decay: the clip comes first) in float64;
    returns (p, m, v, total_norm, coef)."""
    g = np.asarray(g, dtype=np.float64)
    norm = total_norm_ref(g, norm_type)
    coef = clip_coef_ref(norm, max_norm)
    p, m, v = R.adam_step(np.asarray(p, dtype=np.float64), g * coef, m, v, step, lr, wd)
    return p, m, v, norm, coef


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
def test_restatement_equals_torch_clip_then_adam(norm_type):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on float64 CPU tensors over four steps: two whose norm exceeds max_norm (the
    gradient is scaled) and two below it (the coefficient clamps to 1)."""
    rs = np.random.RandomState(4)
    n, lr, wd = 1009, 1e-3, 5e-4
    p0, g0 = rs.standard_normal(n), rs.standard_normal(n)
    scales = (1.0, 0.01, 3.0, 0.02)
    max_norm = 0.1 * total_norm_ref(g0, norm_type)                 # coefficients 0.1, 1, 0.033, 1
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=lr, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    coefs = []
    for step, s in enumerate(scales, 1):
        g = g0 * s
        pt.grad = torch.from_numpy(g.copy())
        tn = torch.nn.utils.clip_grad_norm_([pt], max_norm, norm_type=norm_type)
        opt.step()
        p, m, v, norm, coef = clip_then_adam_ref(p, g, m, v, step, lr, wd, max_norm, norm_type)
        coefs.append(coef)
        assert abs(float(tn) - norm) <= 1e-12 * norm
        np.testing.assert_allclose(pt.grad.numpy(), g * coef, rtol=1e-12, atol=0)
        np.testing.assert_allclose(pt.detach().numpy(), p, rtol=0, atol=1e-13)
    st = opt.state[pt]
    np.testing.assert_allclose(st["exp_avg"].numpy(), m, rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(st["exp_avg_sq"].numpy(), v, rtol=1e-11, atol=1e-18)
    assert coefs[1] == 1.0 and coefs[3] == 1.0 and abs(coefs[0] - 0.1) < 1e-6 and coefs[2] < 0.05


def test_restatement_float32_torch_within_the_gpu_bound():
    """The same two torch calls on float32 tensors stay within the bound the GPU test uses against the restatement (2e-6)."""
    rs = np.random.RandomState(4)
    n = 10007
    p0, g0 = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=1e-3, weight_decay=5e-4)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 4):
        gs = (g0 * step).astype(np.float32)
        pt.grad = torch.from_numpy(gs.copy())
        torch.nn.utils.clip_grad_norm_([pt], 10.0)
        opt.step()
        p, m, v, _, coef = clip_then_adam_ref(p, gs, m, v, step, 1e-3, 5e-4, 10.0)
        assert coef < 0.11
    assert np.max(np.abs(pt.detach().numpy().astype(np.float64) - p)) < 2e-6


# ---------------------------------------------------------------------------------------------------------
# nn.utils
# ---------------------------------------------------------------------------------------------------------
def test_nn_utils_resolution():
    import torch.nn as tnn
    from ctc_pytorch_amd import nn
    assert nn.utils.clip_grad_norm_ is not tnn.utils.clip_grad_norm_ and nn.utils.clip_grad_norm_.__module__ == "ctc_pytorch_amd.nn"
    assert nn.utils.rnn is tnn.utils.rnn
    assert nn.utils.parameters_to_vector is tnn.utils.parameters_to_vector
    assert nn.utils.clip_grad_value_ is tnn.utils.clip_grad_value_
    assert nn.init is tnn.init                                   # the module-level fall-through is untouched
    with pytest.raises(AttributeError):
        nn.utils.no_such_name
    import ctc_pytorch_amd.nn.utils as u                          # importable under its dotted name, too
    assert u is nn.utils


def test_nn_utils_clip_defers_to_torch_for_ordinary_parameters():
    """Parameters that are not homed in a FlatAdam buffer (CPU tensors here) take torch's path, with torch's result."""
    from ctc_pytorch_amd import nn
    rs = np.random.RandomState(0)
    a = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s).astype(np.float32))) for s in ((3, 4), (5,))]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    for pa, pb in zip(a, b):
        pa.grad = torch.from_numpy(rs.standard_normal(tuple(pa.shape)).astype(np.float32))
        pb.grad = pa.grad.clone()
    na = nn.utils.clip_grad_norm_(a, 0.5)
    nb = torch.nn.utils.clip_grad_norm_(b, 0.5)
    assert torch.equal(na, nb) and all(torch.equal(pa.grad, pb.grad) for pa, pb in zip(a, b))
    assert torch.equal(nn.utils.clip_grad_norm_(a[0], 0.1, norm_type=1.0), torch.nn.utils.clip_grad_norm_(b[0], 0.1, norm_type=1.0))
    with pytest.raises(RuntimeError, match="non-finite"):
        a[0].grad[0, 0] = float("nan")
        nn.utils.clip_grad_norm_(a, 0.5, error_if_nonfinite=True)


def test_flat_cover_detection():
    """_flat_grad_of: views that tile one 1-D buffer exactly once -> that buffer; a missing view, a foreign tensor or a partial cover -> None."""
    from ctc_pytorch_amd import nn
    flat = torch.zeros(20)

    def homed(lo, hi, shape):
        p = torch.nn.Parameter(torch.zeros(shape))
        p._ctcn_grad = flat[lo:hi].view(shape)
        return p
    ps = [homed(12, 20, (2, 4)), homed(0, 12, (3, 4))]
    got = nn._flat_grad_of(ps)
    assert got is not None and got.data_ptr() == flat.data_ptr() and got.numel() == 20
    assert nn._flat_grad_of(ps + [ps[0]]) is not None                      # a parameter listed twice is still one view
    assert nn._flat_grad_of(ps[:1]) is None                                 # partial cover
    assert nn._flat_grad_of(ps + [torch.nn.Parameter(torch.zeros(2))]) is None
    other = torch.nn.Parameter(torch.zeros(4))
    other._ctcn_grad = torch.zeros(8)[2:6]
    assert nn._flat_grad_of(ps + [other]) is None and nn._flat_grad_of([]) is None


# ---------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------
def test_run_epoch_allreduces_before_the_clipped_step(monkeypatch):
    """run_epoch on the CPU with the model, the optimiser, the device-side error count and parallel.allreduce_grads stubbed: on every
    step the order is zero_grad, all-reduce of the flat gradient, step -- the clip lives inside step(), so every rank clips the reduced
    gradient -- and the epoch-end line carries the dropped-step count and the last norm when a feature is on."""
    from ctc_pytorch_amd import ops, parallel
    from ctc_pytorch_amd.optim import FlatAdam
    from ctc_pytorch_amd.steps import train_ctc as TR
    events = []
    T, B, V = 6, 2, 5

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(V))

        def forward(self, x):
            return torch.log_softmax(x.transpose(0, 1)[..., :V] + self.w, -1)          # (T,B,V)

    class Opt(FlatAdam):
        def __init__(self, clip):                                                      # no device: FlatAdam.__init__ is not run
            self.grad = torch.zeros(3)
            self.max_grad_norm, self.skip_nonfinite, self.norm_type = (1.0, True, 2.0) if clip else (None, False, 2.0)

        def zero_grad(self, set_to_none=False):
            events.append("zero")

        def step(self):
            events.append("step")

        skipped_steps = property(lambda self: 2)
        last_grad_norm = property(lambda self: torch.tensor(3.5))

    monkeypatch.setattr(parallel, "allreduce_grads", lambda g: events.append("allreduce") or g)
    monkeypatch.setattr(ops, "argmax_last", lambda out: out.argmax(-1).to(torch.int32))
    monkeypatch.setattr(ops, "greedy_collapse", lambda idx, lens, blank=0: (idx.t().contiguous(), torch.full((B,), T, dtype=torch.int32)))
    monkeypatch.setattr(ops, "edit_distance", lambda ids, ids_len, tg, tl: torch.ones(B, dtype=torch.int32))
    data = [(torch.randn(B, T, V), torch.ones(B), torch.ones(B, 2, dtype=torch.int64), torch.full((B,), 2, dtype=torch.int64), ["a", "b"])
            for _ in range(3)]
    for clip in (True, False):
        del events[:]
        lines = []
        TR.run_epoch(1, Model(), data, torch.nn.CTCLoss(reduction="sum"), "cpu", optimizer=Opt(clip), log=lines.append)
        assert events == ["zero", "allreduce", "step"] * 3
        assert ("dropped_steps: 2, last_grad_norm: 3.5" in lines[-1]) == clip, lines[-1]


def test_driver_options_default_off():
    from ctc_pytorch_amd.steps.train_ctc import Config, optimizer_options
    opts = Config()
    assert optimizer_options(opts) == {"max_grad_norm": None, "skip_nonfinite": False}
    opts.max_grad_norm, opts.skip_nonfinite_steps = 400, True                      # the YAML keys
    assert optimizer_options(opts) == {"max_grad_norm": 400.0, "skip_nonfinite": True}
    opts.max_grad_norm, opts.skip_nonfinite_steps = None, False                    # `max_grad_norm: null`
    assert optimizer_options(opts) == {"max_grad_norm": None, "skip_nonfinite": False}


def test_driver_builds_flat_adam_with_the_options(monkeypatch):
    """main() hands exactly optimizer_options() to FlatAdam: without the two keys both features are off."""
    from ctc_pytorch_amd.steps import train_ctc as TR
    seen = []

    class Stop(Exception):
        pass

    def fake(model, **kw):
        seen.append(kw)
        raise Stop()
    monkeypatch.setattr(TR, "FlatAdam", fake)
    class Model(torch.nn.Linear):
        def to(self, *a, **k):                                                       # (the driver's device is a GPU; this test has none)
            return self
    monkeypatch.setattr(TR, "build_model_from_opts", lambda opts, num_class: Model(2, 2))
    base = dict(seed=1, init_lr=1e-3, weight_decay=0.0)
    for extra, want in (({}, (None, False)), ({"max_grad_norm": 400, "skip_nonfinite_steps": True}, (400.0, True))):
        threads = torch.get_num_threads()
        with pytest.raises(Stop):
            TR.main(dict(base, **extra), train_loader=[], dev_loader=[], num_class=5, log=lambda *_: None)
        torch.set_num_threads(threads)
        assert (seen[-1]["max_grad_norm"], seen[-1]["skip_nonfinite"]) == want


def test_flat_adam_rejects_bad_clip_arguments():
    """The argument checks come before anything touches a device."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.optim import FlatAdam
    m = torch.nn.Linear(2, 2)
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FlatAdam(m, max_grad_norm=bad)
    for bad in (1, 1.0, 3, "fro"):
        with pytest.raises(NotImplementedError, match="2 and inf"):
            FlatAdam(m, norm_type=bad)
        with pytest.raises(NotImplementedError, match="2 and inf"):
            ops.norm_type_code(bad)
    assert ops.norm_type_code(2) == 2 and ops.norm_type_code(float("inf")) == 0 and ops.norm_type_code("inf") == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        FlatAdam(m, max_grad_norm=1.0, norm_type=float("inf"), skip_nonfinite=True)          # valid arguments: the usual device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_norm(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clip_grad_norm_(torch.zeros(4), 1.0)
