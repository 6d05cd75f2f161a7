"""The backward recurrences after their cell math was split into a prepare phase (in front of the hand-off wait) and a finish phase (on the
chain): every output bit must be what the commit before the split computed.

tests/golden/rnn_bwd_parent_bits.npz was written by tools/record_rnn_bwd_bits.py from a build of that parent commit (its hash is in the file),
never from the code under test.  Per case it holds y, dx and every weight gradient as float32, and the kernels the parent launched.  An array of
more than FULL_MAX elements (the recurrent weight gradients, mostly: 4H x H floats per direction) is held as the SHA-256 of its bytes plus every
n-th element: the digest decides equality of every bit, the sample gives a failure its count and size; the committed file must stay far below the
repository's size limit.  Inputs come from a seeded numpy generator on the host, the dropout stream starts at 0."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "rnn_bwd_parent_bits.npz")
FULL_MAX = 8192          # elements: larger arrays are stored as digest + sample
SAMPLE = 2048

# name: cell, T, B, I, H, bidirectional, dropout, matmul precision, options for the duration of the case, backward kernel the case is about
CASES = {
    # rnn_bwd_scatter, one tile per exchange wave: a partial batch tile and an odd T against the loop unrolled by two
    "scatter_h64": ("lstm", 5, 20, 8, 64, True, 0.0, 1, {}, "rnn_bwd_scatter"),
    "scatter_h64_dropout": ("lstm", 5, 20, 8, 64, True, 0.3, 1, {}, "rnn_bwd_scatter"),
    # ... two tiles per exchange wave: the flagship instantiation
    "scatter_h320": ("lstm", 4, 16, 8, 320, True, 0.0, 1, {}, "rnn_bwd_scatter"),
    # no gather at step 0, and e1 = 0 at the last step: T = 2 is the shortest sequence the host gives to a persistent kernel (T = 1 runs the
    # per-timestep kernels, whose one-phase cell_bwd is now finish(prepare()): the same check for that form)
    "step_h64_T1": ("lstm", 1, 20, 8, 64, True, 0.0, 1, {}, "rnn_bwd_step"),
    "scatter_h64_T2": ("lstm", 2, 20, 8, 64, True, 0.0, 1, {}, "rnn_bwd_scatter"),
    "scatter_gru": ("gru", 5, 9, 8, 128, True, 0.2, 1, {}, "rnn_bwd_scatter"),
    "scatter_tanh": ("tanh", 3, 20, 8, 48, False, 0.0, 1, {}, "rnn_bwd_scatter"),
    # rnn_bwd_scatter2: forced on the small layer, and where the library picks it
    "scatter2_forced_h64": ("lstm", 5, 20, 8, 64, True, 0.0, 1, {"bwd_item_gather": 2}, "rnn_bwd_scatter2"),
    "scatter2_h384": ("lstm", 4, 8, 8, 384, True, 0.0, 1, {}, "rnn_bwd_scatter2"),
    # the kernels that keep the one-phase call (the split changed the order of their instructions, not the instructions)
    "persist_f32_h64": ("lstm", 4, 16, 8, 64, True, 0.0, 0, {}, "rnn_bwd_persist"),
    "step_h64": ("lstm", 3, 20, 8, 64, True, 0.0, 1, {"rnn_persistent": 0}, "rnn_bwd_step"),
}
ARRAYS = ("y", "dx", "dw_ih0", "dw_hh0", "dw_ih1", "dw_hh1")


def make_inputs(name):
    cell, T, B, I, H, bi, _, _, _, _ = CASES[name]
    G = {"lstm": 4, "gru": 3, "tanh": 1}[cell]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    f = lambda *shape: rng.standard_normal(shape, dtype=np.float32)
    x = f(T, B, I)
    w = [f(G * H, I) * np.float32(0.2), f(G * H, H) * np.float32(1.0 / H ** 0.5)]
    w += [f(G * H, I) * np.float32(0.2), f(G * H, H) * np.float32(1.0 / H ** 0.5)] if bi else [None, None]
    dy = f(T, B, (2 if bi else 1) * H)
    return x, w, dy


def run_case(name, dev):
    """-> ({array name: float32 numpy array}, (forward kernel, backward kernel))"""
    from ctc_pytorch_amd import ops
    cell, T, B, I, H, bi, drop, prec, opts, _ = CASES[name]
    x, w, dy = make_inputs(name)
    before = {k: ops.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        ops.set_precision(prec)
        torch.manual_seed(11)                 # the dropout's Philox seed is torch.initial_seed(); nothing else here draws from torch's generator
        ops._drop_counter[0] = 0
        xs = torch.from_numpy(x).to(dev).requires_grad_(True)
        ws = [torch.from_numpy(t).to(dev).requires_grad_(True) if t is not None else None for t in w]
        y = ops.rnn_layer(xs, ws[0], ws[1], ws[2], ws[3], cell, True, drop)
        y.backward(torch.from_numpy(dy).to(dev))
        torch.cuda.synchronize()
        ops.check_health(dev)
        kernels = ops.rnn_last_kernels()[:2]
    finally:
        for k, v in before.items():
            ops.set_option(k, v)
    out = {"y": y.detach(), "dx": xs.grad}
    for key, t in zip(ARRAYS[2:], ws):
        if t is not None:
            out[key] = t.grad
    return {k: v.cpu().numpy().astype(np.float32, copy=False) for k, v in out.items()}, tuple(kernels)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sample_of(a):
    flat = a.reshape(-1)
    return flat[:: max(1, flat.size // SAMPLE)]


@pytest.fixture(scope="module")
def parent():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def test_fixture_covers_every_case(parent):
    arrays, meta = parent
    assert len(meta["commit"]) >= 7 and sorted(meta["kernels"]) == sorted(CASES)
    for name, case in CASES.items():
        assert meta["kernels"][name][1] == case[9], (name, meta["kernels"][name])
        for key in ARRAYS:
            if case[5] or not key.endswith("1"):
                assert "%s/%s" % (name, key) in arrays or "%s/%s.sha256" % (name, key) in meta["digests"], (name, key)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rnn_bits_are_the_parents(parent, dev, name):
    arrays, meta = parent
    got, kernels = run_case(name, dev)
    assert list(kernels) == meta["kernels"][name], "the case moved to other kernels: %s, the parent ran %s" % (kernels, meta["kernels"][name])
    assert kernels[1] == CASES[name][9], kernels
    bad = []
    for key, g in got.items():
        full, dkey = "%s/%s" % (name, key), "%s/%s.sha256" % (name, key)
        if full in arrays:
            want = arrays[full]
            assert want.dtype == np.float32 and want.shape == g.shape, (key, want.shape, g.shape)
            if not torch.equal(torch.from_numpy(g), torch.from_numpy(want)):
                d = np.abs(g.astype(np.float64) - want.astype(np.float64))
                bad.append("%s: %d of %d elements differ, max |diff| %.3e" % (key, int((g != want).sum()), g.size, float(np.nanmax(d))))
        else:
            want = arrays[full + ".sample"]
            s = sample_of(g)
            if digest(g) != meta["digests"][dkey]:
                d = np.abs(s.astype(np.float64) - want.astype(np.float64))
                bad.append("%s: digest of the %d elements differs; of the %d sampled ones %d differ, max |diff| %.3e"
                           % (key, g.size, s.size, int((s != want).sum()), float(np.nanmax(d))))
            else:
                assert torch.equal(torch.from_numpy(np.ascontiguousarray(s)), torch.from_numpy(want))
    assert not bad, "; ".join(bad)
    expected = {k for k in ARRAYS if CASES[name][5] or not k.endswith("1")}
    assert set(got) == expected, (sorted(got), sorted(expected))
