"""The seven recurrence kernels of rnn.hip against float64, outside the linear regime.

Everywhere else in the suite the recurrent layer runs with small weights: gate pre-activations of std 0.2-0.5, sigmoid = 1/2 + a/4, tanh = a,
forget / update gates near 1/2, |c| < 0.3, nothing remembered for more than ~15 frames.  A trained model does not live there.  Two families
of tests, both against tests/rnn_cell_ref.py (numpy float64; tests/test_rnn_regimes_host.py holds it to torch's float64 layers to 1e-12):

1. Trained-regime LAYERS (`test_layer_*`): a torch-default-initialised layer pushed into saturation through its input projection (`input16`,
   `input64`, `mixed`) or given per-unit forget / update biases of 2-8 (`memory`), W_hh untouched -- the host tests check that each regime is
   as saturated / long-lived as it says and that torch's own float32 layer stays within 4e-6 (y) / 5e-6 (gradients, rel-L2) of its float64
   self there, which is what the gates below rest on: precision 0  max|dy| < 2e-5, rel-L2 < 1e-4 (the gates of test_rnn_layer_vs_torch_cpu
   in the linear regime);  precision 1  1e-3, 5e-4 (GATES below says why the output gate is SURVEY 8a's and not the linear regime's 1e-4).
   Every (regime, shape) runs on every kernel pair that takes it, and the kernel that ran is asserted.
   Shapes (T, B, I, H), the smallest that reach each code path:
     48,  5,  8,  32   one partial batch tile, two 16-unit slices, one tagged pair
     48, 17, 16,  72   a second batch tile with one row; H % 32 != 0: rnn_fwd_persist at precision 1, last backward slice padded
     24,  9, 16, 320   the benchmark width: 20 slices, rnn_bwd_scatter at two tiles per scattering wave
     24,  9, 16, 384   24 slices: rnn_bwd_scatter2 by default, rnn_bwd_scatter's and the one-pass tagged forward's limit
     12, 33,  8, 512   cfg4's width: three batch tiles, reserve traffic through LDS in the tagged forward, kq = 8
   plus one single-direction case per gated cell, the tanh cell at the first two shapes and one batch-chunked layer (B = 144).

2. The pointwise SWEEP (`test_sweep_*`): ctcn_rnn_fwd_ex / ctcn_rnn_bwd_ex called directly, so that the reserves `gates` and `aux` -- contract
   of include/ctcn.h, never compared with anything before -- are visible.  Inputs are designed so that every pre-activation is known
   exactly (rnn_cell_ref.sweep_case: a_g = s_j * x_g with s_j a power of two and x on a 12-bit grid from 2^-20 to 3e38), with W_hh = 0 (the
   activations and the carried c / h / dc / dh*z alone) or 0.5 * I per gate block (e1 terms and the GRU's r * (W_hn h) live).  Each saved
   activation must be within the source's own claim (3e-7 absolute) of float64, everything downstream within a per-element bound DERIVED
   from that claim by running error analysis (rnn_cell_ref.sweep_bounds), and the saturated ends must come out exact.
   Not observable here: "-0 stays -0 through tanh".  A pre-activation reaches act_tanh as (recurrent sum) + (projection), and both the
   GEMM's accumulator and that sum turn -0 into +0; the host test checks the formula's sign handling instead, this one that a zero
   pre-activation gives a zero.  The tanh cell saves no activations in `gates` (its kernels read h from y), so its forward reserve is not
   compared.

CTCN_REGIME_LOG=<file>: one JSON line per case with the measured distances (the record the figures in the commit message come from).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnn_cell_ref as R  # noqa: E402

gpu = pytest.mark.gpu
ALL_KERNELS = {"rnn_fwd_step", "rnn_fwd_persist", "rnn_fwd_tagged", "rnn_bwd_step", "rnn_bwd_persist", "rnn_bwd_scatter", "rnn_bwd_scatter2"}

# kernel pairs, by the switches the suite already uses: (precision, rnn_persistent, option rnn_fwd_tagged, option bwd_item_gather)
CONFIGS = {
    "step_f32": (0, 0, 1, 1),
    "step_bf16": (1, 0, 1, 1),            # the per-timestep kernels multiply in f32 at either precision: only the projection is bf16x3
    "persist_f32": (0, 1, 1, 1),
    "tagged_scatter": (1, 1, 1, 0),
    "persist_gather": (1, 1, 0, 2),
    "default": (1, 1, 1, 1),
}


def expected_kernels(config, cell, H):
    """The dispatch rules of rnn.hip (tagged_gather_applies, bwd_choose_formulation) for the shapes of this file: all co-resident."""
    prec, persistent, tagged, gather = CONFIGS[config]
    if not persistent:
        return "rnn_fwd_step", "rnn_bwd_step"
    if prec == 0:
        return "rnn_fwd_persist", "rnn_bwd_persist"
    nsl = (H + 15) // 16
    fwd = "rnn_fwd_tagged" if (tagged and cell != "tanh" and H % 32 == 0) else "rnn_fwd_persist"
    if gather == 2 or (gather == 1 and nsl > 20):
        return fwd, "rnn_bwd_scatter2"
    return fwd, ("rnn_bwd_scatter" if nsl <= 24 else "rnn_bwd_persist")


def _layer_table():
    """[(case key, config, (forward kernel, backward kernel))]: every case on every kernel pair that differs for it"""
    table = []
    for key in R.layer_cases():
        cell, H = key[0], key[5]
        if key[3] > 64:
            continue                                   # the batch-chunk case has its own test
        seen = set()
        for config in CONFIGS:
            pair = expected_kernels(config, cell, H)
            if (CONFIGS[config][0], pair) not in seen:
                seen.add((CONFIGS[config][0], pair))
                table.append((key, config, pair))
    return table


LAYER_TABLE = _layer_table()
SWEEP_TABLE = [(cell, H, whh, config, expected_kernels(config, cell, H))
               for cell in ("lstm", "gru", "tanh") for H in (32, 64) for whh in (0.0, 0.5) for config in ("step_f32", "persist_f32", "tagged_scatter", "persist_gather")]


class SplitFigureMissed(AssertionError):
    """rnn_fwd_tagged carries h less exactly than the 2^-16 the project states for a bf16x3 operand"""


# The sweep cases in which rnn_fwd_tagged misses the bound built on the STATED split figure (2^-16 relative) while it meets the one built
# on what its hand-off can lose by construction (rnn_cell_ref.SPLIT_TAGGED = 1.5 * 2^-16: both planes rounded to nearest, then the step
# tag written over the LSB of lo).  Measured: saved activations 1.02x (LSTM, H = 64), W_hn h 1.12x (GRU, H = 32) and 1.33x (GRU, H = 64)
# their bounds, e.g. W_hn h = 0.285728455 for 0.285733806, 5.35e-6 off where 4.77e-6 is allowed.  Rounding lo to its free bits would meet
# the figure, but it changes every h the kernel hands on, i.e. the bits of every precision-1 golden and checksum of the linear regime, and
# adds an instruction to the serial path of the step: not done here.  strict: the mark falls once the kernel or its stated figure moves.
TAG_COSTS_MORE_THAN_STATED = {("lstm", 64, 0.5, "tagged_scatter"), ("gru", 32, 0.5, "tagged_scatter"), ("gru", 64, 0.5, "tagged_scatter")}
_XFAIL = pytest.mark.xfail(strict=True, raises=SplitFigureMissed,
                           reason="rnn_fwd_tagged: the step tag in the LSB of lo on top of the two roundings loses up to 1.5 * 2^-16 of h, not the stated 2^-16; "
                                  "measured 1.02-1.33x the derived bound on the saved activations / W_hn h; a fix changes the linear-regime bits")


def test_every_recurrence_kernel_is_covered():
    """A later edit of the tables cannot silently drop a kernel: each family names all seven, at both precisions where the kernel has both."""
    for table, pair_of in ((LAYER_TABLE, lambda e: e[2]), (SWEEP_TABLE, lambda e: e[4])):
        names = set()
        for e in table:
            names.update(pair_of(e))
        assert names == ALL_KERNELS, sorted(ALL_KERNELS - names)
    for regime in R.REGIMES:
        for cell in ("lstm", "gru"):
            names = set()
            for key, _, pair in LAYER_TABLE:
                if key[0] == cell and key[1] == regime:
                    names.update(pair)
            assert names == ALL_KERNELS, (cell, regime, sorted(ALL_KERNELS - names))
    assert {k[:2] for k, _, _ in LAYER_TABLE} >= {("tanh", r) for r in R.regimes_of("tanh")}
    assert any(k[6] == 1 for k, _, _ in LAYER_TABLE)
    assert {k[2:6] for k, _, _ in LAYER_TABLE} >= set(R.SHAPES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


class _switches(object):
    """precision, rnn_persistent, rnn_fwd_tagged, bwd_item_gather for the duration of a `with`, then exactly what was there before"""

    def __init__(self, config):
        self.want = CONFIGS[config]

    def __enter__(self):
        from ctc_pytorch_amd import ops
        self.old = (ops.get_precision(), ops.get_option("rnn_persistent"), ops.get_option("rnn_fwd_tagged"), ops.get_option("bwd_item_gather"))
        self._set(self.want)

    def __exit__(self, *exc):
        self._set(self.old)

    @staticmethod
    def _set(v):
        from ctc_pytorch_amd import ops
        ops.set_precision(v[0])
        ops.set_rnn_persistent(v[1])
        ops.set_option("rnn_fwd_tagged", v[2])
        ops.set_option("bwd_item_gather", v[3])


def _log(record):
    path = os.environ.get("CTCN_REGIME_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def _t(a, dev):
    return torch.tensor(a, dtype=torch.float32, device=dev)


def _layer_distances(dev, key, y, xg, ws):
    """(max|dy|, {gradient: rel-L2}) of a finished layer run against the float64 reference; everything finite"""
    _, ref = R.layer_case(key)
    got = [("dx", xg.grad)] + [(n, w.grad) for (n, _), w in zip(R.gradients(ref)[1:], ws)]
    assert torch.isfinite(y).all()
    for n, g in got:
        assert torch.isfinite(g).all(), n
    dist = {n: R.rel_l2(g.cpu().numpy(), want) for (n, g), (_, want) in zip(got, R.gradients(ref))}
    return R.max_abs(y.detach().cpu().numpy(), ref["y"]), dist


def _layer_inputs(dev, key):
    case, _ = R.layer_case(key)
    dirs = key[6]
    xg = _t(case["x"], dev).requires_grad_(True)
    ws = []
    for d in range(dirs):
        ws += [_t(case["w_ih"][d], dev).requires_grad_(True), _t(case["w_hh"][d], dev).requires_grad_(True)]
    return xg, ws, _t(case["dy"], dev)


# (max|dy|, gradient rel-L2) per precision.  Precision 0: the gates of test_rnn_layer_vs_torch_cpu.  Precision 1: the gradient gate of
# test_rnn_layer_bf16x3_vs_torch_cpu; its OUTPUT gate, 1e-4, is out of reach here and SURVEY 8a's 1e-3 for the bf16-operand mode applies
# instead -- see test_layer_in_trained_regime_vs_float64.
GATES = {0: (2e-5, 1e-4), 1: (1e-3, 5e-4)}


@gpu
@pytest.mark.parametrize("key,config,pair", LAYER_TABLE, ids=["%s-%s-T%dB%dI%dH%dx%d-" % k + c for k, c, _ in LAYER_TABLE])
def test_layer_in_trained_regime_vs_float64(dev, key, config, pair):
    """Measured on an MI355X, worst case per regime over all cells, shapes and kernel pairs (max|dy| / worst gradient rel-L2):
                   precision 0            precision 1
      input16      1.1e-6 / 4.3e-7        1.0e-4 / 2.2e-5
      input64      3.4e-6 / 8.0e-7        4.4e-4 / 9.9e-5
      mixed        2.4e-6 / 5.5e-7        2.0e-4 / 4.6e-5
      memory       8.4e-7 / 3.5e-6        1.1e-4 / 5.6e-5
    Precision 0 sits where torch's own float32 layer sits (host test: up to 3.4e-6 / 3.6e-6).  Precision 1 does not meet the 1e-4 output
    gate of the linear regime: the worst case, tanh input64 T=48 B=5 I=8 H=32, is 4.4e-4 from float64 on every precision-1 kernel pair,
    where the precision-0 kernels are 2.5e-6 away and torch float32 2.5e-6.  That is the bf16x3 input projection, not the recurrence: a
    pre-activation there is a sum of 8 products of magnitude ~10-30 that cancel, each carried to ~2^-17, so it is known to a few 1e-4 and
    tanh's slope is 1 where they cancel.  Precision 1 is therefore held to SURVEY 8a's 1e-3 on outputs (2.3x the worst case) and keeps
    the 5e-4 gradient gate (5x)."""
    from ctc_pytorch_amd import ops
    cell = key[0]
    xg, ws, dy = _layer_inputs(dev, key)
    w4 = ws + [None, None] * (2 - key[6])
    with _switches(config):
        y = ops.rnn_layer(xg, w4[0], w4[1], w4[2], w4[3], cell)
        y.backward(dy)
        torch.cuda.synchronize()
        ran = ops.rnn_last_kernels()
    ops.check_health(dev)
    assert ran == pair, (ran, pair)
    prec = CONFIGS[config][0]
    dy_, dist = _layer_distances(dev, key, y, xg, ws)
    _log({"test": "layer", "cell": cell, "regime": key[1], "shape": key[2:], "config": config, "precision": prec, "kernels": ran, "y": dy_, "grad": dist})
    print("%s %s: max|dy| %.2e  rel-L2 %s" % (key, ran, dy_, {n: "%.1e" % v for n, v in dist.items()}))
    assert dy_ < GATES[prec][0]
    for n, v in dist.items():
        assert v < GATES[prec][1], (n, v)


@gpu
def test_layer_with_long_memory_in_batch_chunks_vs_float64(dev):
    """B = 144 at H = 320: no persistent launch holds it, so the layer runs as batch chunks (64 + 64 + 16 rows), one persistent launch each --
    the carried state must start from zero in every chunk and the weight gradients add up across them.  `memory`, LSTM, precision 1."""
    from ctc_pytorch_amd import _lib, ops
    key = ("lstm", "memory") + R.CHUNK_SHAPE + (2,)
    T, B, I, H = R.CHUNK_SHAPE
    L = _lib.lib()
    limit = ops.persistent_batch_limit(H, 2, L.ctcn_device_xcds(), L.ctcn_device_cus())
    assert 0 < limit < B, limit
    xg, ws, dy = _layer_inputs(dev, key)
    mark = (R.CELLS["lstm"], H, 2, B)
    had, chunks_on = mark in ops._fallback_shapes, ops._chunks_on[0]
    try:
        ops.set_batch_chunks(True)
        ops.mark_batch_chunks("lstm", H, 2, B)
        with _switches("default"):
            y = ops.rnn_layer(xg, ws[0], ws[1], ws[2], ws[3], "lstm")
            y.backward(dy)
            torch.cuda.synchronize()
            ran = ops.rnn_last_kernels()
    finally:
        ops.set_batch_chunks(chunks_on)
        if not had:
            ops._fallback_shapes.discard(mark)
    ops.check_health(dev)
    assert ran == ("rnn_fwd_tagged", "rnn_bwd_scatter"), ran
    dy_, dist = _layer_distances(dev, key, y, xg, ws)
    _log({"test": "chunks", "cell": "lstm", "regime": "memory", "shape": key[2:], "config": "default", "precision": 1, "kernels": ran, "y": dy_, "grad": dist})
    print("%s %s: max|dy| %.2e  rel-L2 %s" % (key, ran, dy_, {n: "%.1e" % v for n, v in dist.items()}))
    assert dy_ < GATES[1][0]
    for n, v in dist.items():
        assert v < GATES[1][1], (n, v)


# ---- the pointwise sweep -----------------------------------------------------------------------------------------------------------
def _abi_run(dev, cell, case, prec):
    """ctcn_rnn_fwd_ex, then ctcn_rnn_bwd_ex without weight gradients, on the current stream.  Returns the tensors of the ABI as float64
    numpy -- act / aux (reserves after forward), y, da / daux (reserves after backward), dx -- and the kernels the two calls launched."""
    from ctc_pytorch_amd import _lib, ops
    L = _lib.lib()
    code, G = R.CELLS[cell], R.GATES[cell]
    T, B, I = case["x"].shape
    H = case["w_hh"][0].shape[1]
    x, dy = _t(case["x"], dev), _t(case["dy"], dev)
    w_ih = _t(np.concatenate(case["w_ih"]), dev)                  # [W_ih fwd ; W_ih rev] stacked
    w_hh = [_t(w, dev) for w in case["w_hh"]]
    y = torch.empty(T, B, 2 * H, device=dev)
    gates = torch.empty(T, B, 2, G * H, device=dev)
    aux = torch.empty(T, B, 2, H, device=dev) if cell != "tanh" else None
    dx = torch.empty_like(x)
    scratch = torch.empty(L.ctcn_rnn_scratch_bytes(code, B, H, 2), dtype=torch.uint8, device=dev)
    _, wp, wn = ops._ws(x)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(_lib.stream_ptr())
    call, fwd_name = ops._new_rnn_call(dev)
    _lib.check(L.ctcn_rnn_fwd_ex(code, T, B, I, H, 2, P(x), P(w_ih), P(w_hh[0]), P(w_ih[G * H:]), P(w_hh[1]), P(y), P(gates), P(aux), prec, wp, wn, st,
                                 ctypes.byref(call)), "rnn_fwd_ex")
    torch.cuda.synchronize()
    n64 = lambda t: t.detach().cpu().numpy().astype(np.float64) if t is not None else None
    out = {"act": n64(gates), "aux": n64(aux), "y": n64(y), "y32": y.cpu().numpy(), "act32": gates.cpu().numpy()}
    call2, bwd_name = ops._new_rnn_call(dev)
    _lib.check(L.ctcn_rnn_bwd_ex(code, T, B, I, H, 2, P(x), P(w_ih), P(w_hh[0]), P(w_ih[G * H:]), P(w_hh[1]), P(y), P(gates), P(aux), P(dy), P(dx),
                                 None, None, None, None, 0.0, prec, P(scratch), wp, wn, st, ctypes.byref(call2)), "rnn_bwd_ex")
    torch.cuda.synchronize()
    out.update({"da": n64(gates), "daux": n64(aux), "dx": n64(dx)})
    return out, ((fwd_name.value or b"").decode(), (bwd_name.value or b"").decode())


_sweep_ref = {}


def _sweep(cell, H, whh, prec):
    """(case, float64 reference, values with derived bounds): once per (cell, H, whh, precision), shared, never written to"""
    k = (cell, H, whh)
    if k not in _sweep_ref:
        case = R.sweep_case(cell, H, whh)
        _sweep_ref[k] = (case, R.run(cell, case), {})
    case, ref, bounds = _sweep_ref[k]
    if prec not in bounds:
        bounds[prec] = R.sweep_bounds(cell, case, prec)
    return case, ref, bounds[prec]


@gpu
@pytest.mark.parametrize("cell,H,whh,config,pair", [pytest.param(*e, id="%s-H%d-whh%.1f-%s" % e[:4], marks=[_XFAIL] if e[:4] in TAG_COSTS_MORE_THAN_STATED else [])
                                                    for e in SWEEP_TABLE])
def test_sweep_cell_math_and_reserves_vs_float64(dev, cell, H, whh, config, pair):
    """Measured on an MI355X: every saved activation within 7.7e-8 of float64 where the pre-activation is exact (claim: 3e-7), on all
    three forward kernels; everything else within 0.81 of its derived bound (dx within 0.12), except rnn_fwd_tagged with a live W_hh
    (above; its worst case that still passes, LSTM at H = 32, is at 0.996)."""
    from ctc_pytorch_amd import ops
    prec = CONFIGS[config][0]
    case, ref, bound = _sweep(cell, H, whh, prec)
    with _switches(config):
        got, ran = _abi_run(dev, cell, case, prec)
    ops.check_health(dev)
    assert ran == pair, (ran, pair)
    G = R.GATES[cell]
    checked = ["y", "da", "dx"] + (["act", "aux"] if cell != "tanh" else []) + (["daux"] if cell == "gru" else [])
    for k in ("act", "aux", "y", "da", "daux", "dx"):
        if got[k] is not None:
            # no NaN anywhere, checked tensor or not (the tanh cell's forward reserve is the projection itself: 3e38 * 16 is inf there)
            assert not np.any(np.isnan(got[k])) and (np.all(np.isfinite(got[k])) or (cell, k) == ("tanh", "act")), k + ": not finite"
    worst, missed = {}, None
    for k in checked:
        err = np.abs(got[k] - bound[k].v)
        ratio = err / np.maximum(bound[k].e, 1e-300)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        worst[k] = (float(err.max()), float(ratio[at]))
        if ratio[at] > 1.0:
            text = "%s%s: device %.9g, float64 %.9g, |difference| %.3g above the derived bound %.3g" % (
                k, tuple(int(i) for i in at), got[k][at], bound[k].v[at], err[at], bound[k].e[at])
            # the one known way past a bound: the tagged forward's hand-off of h (TAG_COSTS_MORE_THAN_STATED); held to what it can lose
            # by construction here, reported as a miss of the stated figure once every other check of this case has run
            by_construction = R.sweep_bounds(cell, case, prec, R.SPLIT_TAGGED)[k].e
            assert ran[0] == "rnn_fwd_tagged" and whh != 0.0 and np.all(err <= by_construction), text
            missed = missed or text
    _log({"test": "sweep", "cell": cell, "H": H, "whh": whh, "config": config, "precision": prec, "kernels": ran,
          "worst": {k: {"abs": v[0], "of_bound": v[1]} for k, v in worst.items()}})
    print("%s H=%d whh=%.1f %s: worst |error| (share of its bound) %s" % (cell, H, whh, ran, {k: "%.1e (%.4f)" % v for k, v in worst.items()}))
    # the saved activations themselves: the source's claim, 3e-7 absolute, where the pre-activation is exact (W_hh = 0)
    if whh == 0.0 and cell != "tanh":
        assert np.all(bound["act"].e == R.ACT_EPS) and np.max(np.abs(got["act"] - ref["act"])) <= 3e-7
    # hard edges, on the float32 values as stored
    pre = ref["pre"]
    act = got["act32"] if cell != "tanh" else got["y32"].reshape(pre.shape)
    sig_blocks = {"lstm": (0, 1, 3), "gru": (0, 1), "tanh": ()}[cell]
    tanh_block = {"lstm": 2, "gru": 2, "tanh": 0}[cell]
    n_edge = 0
    for j in sig_blocks:
        a, v = pre[..., j * H:(j + 1) * H], act[..., j * H:(j + 1) * H]
        sat = np.abs(a) >= 1000
        n_edge += int(sat.sum())
        assert np.array_equal(v[sat], (a[sat] > 0).astype(np.float32)), "sigmoid beyond |a| = 1000 is not exactly 0 / 1"
        assert np.any(np.abs(a) > 1e38) and np.any(sat & (a > 0)) and np.any(sat & (a < 0))
    a, v = pre[..., tanh_block * H:(tanh_block + 1) * H], act[..., tanh_block * H:(tanh_block + 1) * H]
    sat = np.abs(a) >= 16
    assert sat.sum() > 100 and np.array_equal(v[sat], np.sign(a[sat]).astype(np.float32)), "tanh beyond |a| = 16 is not exactly +-1"
    zero = a == 0
    assert zero.sum() > 0 and np.all(v[zero] == 0), "tanh of a zero pre-activation is not zero"
    assert G == 1 or n_edge > 100
    if missed:
        raise SplitFigureMissed(missed)
