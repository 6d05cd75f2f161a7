"""The wave-skewed CTC lattice (ctc.hip: ctc_lattices_skew_kernel, option "ctc_lattice_skew" = 1) against the classic kernels
("ctc_lattice_skew" = 0) on the same tensors in the same process, bit for bit: alpha, beta, nll, the gradient of ctcn_ctc_grad_ex and the NaN
patterns, for ctcn_ctc_fwd_ex with beta and alpha-only.  The lattices are pre-filled with a sentinel and compared whole, so a cell that one
kernel writes and the other does not shows as a difference too.

The shapes are the smallest at which the scheme can go wrong: lattices that end on either side of a wave edge (S = 63, 65, 127, 129, 255),
utterances that leave the upper waves without a state, the skip rule across lanes 63 | 0, input lengths around the pipeline's fill and drain
(the skew k and (W - 1) k), a prefetch window that does not divide the length, and one wave at a time delayed by several frames' worth of
sleep ("ctc_slow_wave")."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _log_probs(seed, T, B, V):
    rs = np.random.RandomState(seed)
    return torch.log_softmax(torch.from_numpy((2 * rs.standard_normal((T, B, V))).astype(np.float32)), -1)


def _labels(seed, B, Lmax, V, blank):
    """Random labels from the classes other than `blank`, no two neighbours equal (repeats are set by hand where a case wants them)."""
    rs = np.random.RandomState(seed)
    tg = np.zeros((B, max(Lmax, 1)), dtype=np.int64)[:, :Lmax]
    for i in range(B):
        prev = -1
        for j in range(Lmax):
            c = int(rs.randint(0, V - 1))
            c += c >= blank
            while c == prev:
                c = int(rs.randint(0, V - 1))
                c += c >= blank
            tg[i, j] = prev = c
    return tg


def _run(dev, lp, tg, il, tl, blank=0, with_beta=True, skew=1, slow=0, zero_infinity=0):
    """ctcn_ctc_fwd_ex (+ ctcn_ctc_grad_ex with beta) under the given options -> dict of CPU tensors; the options are put back."""
    from ctc_pytorch_amd import _lib, ops
    T, B, V = lp.shape
    Lmax = tg.shape[1]
    lp_d, il_d, tl_d = lp.to(dev).contiguous(), torch.as_tensor(il, dtype=torch.int64).to(dev), torch.as_tensor(tl, dtype=torch.int64).to(dev)
    tg_d = torch.as_tensor(tg, dtype=torch.int64).to(dev).contiguous()
    L, P, st = _lib.lib(), (lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None), _lib.stream_ptr()
    alpha = torch.full((T, B, 2 * Lmax + 1), SENTINEL, device=dev)
    beta = torch.full_like(alpha, SENTINEL) if with_beta else None
    nll = torch.full((B,), SENTINEL, device=dev)
    old = ops.get_option("ctc_lattice_skew"), ops.get_option("ctc_slow_wave")
    try:
        ops.set_option("ctc_lattice_skew", skew)
        ops.set_option("ctc_slow_wave", slow)
        _lib.check(L.ctcn_ctc_fwd_ex(P(lp_d), P(tg_d), P(il_d), P(tl_d), P(alpha), P(beta), P(nll), T, B, V, Lmax, blank, st), "ctc_fwd_ex")
    finally:
        ops.set_option("ctc_lattice_skew", old[0])
        ops.set_option("ctc_slow_wave", old[1])
    out = {"alpha": alpha, "nll": nll}
    if with_beta:
        gs = torch.full((1,), 1.0 / B, device=dev)
        grad = torch.full_like(lp_d, SENTINEL)
        _lib.check(L.ctcn_ctc_grad_ex(P(lp_d), P(tg_d), P(il_d), P(tl_d), P(alpha), P(beta), P(nll), P(gs), 0, 2, zero_infinity, blank, P(grad),
                                      T, B, V, Lmax, st), "ctc_grad_ex")
        out.update(beta=beta, grad=grad)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _assert_same(ref, got, what=""):
    for k in ref:
        assert _same_bits(ref[k], got[k]), "%s: %s differs in %d cells" % (what, k, int((_bits(ref[k]) != _bits(got[k])).sum()))
        assert torch.equal(torch.isnan(ref[k]), torch.isnan(got[k])), (what, k)


def _check_defined_cells(res, il, tl, T):
    """Exactly the cells t < in_len, s < 2 L + 1 are written (valid lengths); the others keep the sentinel."""
    for k in ("alpha", "beta"):
        if k not in res:
            continue
        a = res[k]
        for i in range(a.shape[1]):
            Tb, S = int(il[i]), 2 * int(tl[i]) + 1
            if not (0 <= Tb <= T and 0 <= int(tl[i]) <= (a.shape[2] - 1) // 2):
                assert bool((a[:, i, :] == SENTINEL).all()), (k, i)          # lengths outside the tensors: nothing is written
                continue
            assert bool((a[:Tb, i, :S] != SENTINEL).all()), (k, i)
            assert bool((a[Tb:, i, :] == SENTINEL).all()) and bool((a[:, i, S:] == SENTINEL).all()), (k, i)


def _both_passes(dev, lp, tg, il, tl, blank=0, what="", **kw):
    from ctc_pytorch_amd import ops
    assert ops.ctc_lattice_plan(tg.shape[1])["skewed"] == 1
    for with_beta in (False, True):                                       # (the result returned is the one with beta and the gradient)
        ref = _run(dev, lp, tg, il, tl, blank, with_beta, skew=0, **kw)
        got = _run(dev, lp, tg, il, tl, blank, with_beta, skew=1, **kw)
        _assert_same(ref, got, "%s beta=%s" % (what, with_beta))
        _check_defined_cells(got, il, tl, lp.shape[0])
    return got


def _edge_batch(Lmax, V=20, blank=0, seed=0):
    """B = 8: full length (0), L = 0 (1), L = 1 (2), L = 5: the upper waves hold no state (3), repeats at label positions 30-33 and 62-65, i.e.
    states 61-67 and 125-131 across lanes 63 | 0 (4), distinct labels there (5), one label repeated over the whole string (6), ragged (7)."""
    B, T = 8, 2 * Lmax + 6
    tg = _labels(seed + Lmax, B, Lmax, V, blank)
    tl = np.array([Lmax, 0, 1, min(5, Lmax), Lmax, Lmax, Lmax, max(Lmax - 3, 0)], dtype=np.int64)
    il = np.array([T, T, T - 1, T - 2, T, T - 3, T, T // 2 + 1], dtype=np.int64)
    other = [c for c in range(V) if c != blank]
    for lo in (30, 62):
        for j in range(lo, min(lo + 4, Lmax)):
            tg[4, j] = other[3]
            tg[5, j] = other[j - lo]
    tg[6, :] = other[1]
    return T, B, V, tg, il, tl


@pytest.mark.parametrize("Lmax", [31, 32, 63, 64, 127])
def test_wave_edges_and_skip_rule(dev, Lmax):
    from ctc_pytorch_amd import ops
    T, B, V, tg, il, tl = _edge_batch(Lmax)
    assert ops.ctc_lattice_plan(Lmax)["waves"] == -(-(2 * Lmax + 1) // 64)
    got = _both_passes(dev, _log_probs(Lmax, T, B, V), tg, il, tl, what="Lmax %d" % Lmax)
    assert bool(torch.isfinite(got["nll"][[0, 1, 2, 3, 5]]).all())       # the cases are real alignments, not lattices of -inf


def test_dispatch_edge_takes_the_classic_path(dev):
    from ctc_pytorch_amd import ops
    Lmax = 128
    assert ops.ctc_lattice_plan(127)["skewed"] == 1 and ops.ctc_lattice_plan(Lmax)["skewed"] == 0
    T, B, V, tg, il, tl = _edge_batch(Lmax)
    lp = _log_probs(5, T, B, V)
    for with_beta in (True, False):
        _assert_same(_run(dev, lp, tg, il, tl, 0, with_beta, skew=0), _run(dev, lp, tg, il, tl, 0, with_beta, skew=1), "Lmax 128")


@pytest.mark.parametrize("Lmax", [64, 127])
def test_fill_and_drain(dev, Lmax):
    """Input lengths around the pipeline's fill and drain, with every wave holding states (full-length labels) and with mixed label lengths."""
    from ctc_pytorch_amd import ops
    p = ops.ctc_lattice_plan(Lmax)
    k, W, T, V = p["skew"], p["waves"], 40, 20
    lens = [0, 1, 2, 3, k, k + 1, (W - 1) * k, (W - 1) * k + 1, T, 4, 5, 6, 9]    # (the last four: around the 4-frame chunks of the hand-off)
    B = len(lens)
    tg = _labels(7, B, Lmax, V, 0)
    il = np.array(lens, dtype=np.int64)
    lp = _log_probs(11 + Lmax, T, B, V)
    _both_passes(dev, lp, tg, il, np.full(B, Lmax, dtype=np.int64), what="full labels")
    tl = np.array([Lmax, 1, 0, 2, 1, 3, 2, 3, 20, 2, Lmax, 3, 4], dtype=np.int64)[:B]      # feasible where the input is long enough
    got = _both_passes(dev, lp, tg, il, tl, what="mixed labels")
    assert bool(torch.isfinite(got["nll"][[8, 7, 6, 4, 3]]).all())


def test_first_small_case(dev):
    """The smallest fill / drain case (T = 40, Lmax = 64, B = 2): three waves, one utterance of full length and one that leaves two waves empty."""
    T, B, V, Lmax = 40, 2, 20, 64
    tg = _labels(1, B, Lmax, V, 0)
    _both_passes(dev, _log_probs(1, T, B, V), tg, np.array([T, 7]), np.array([Lmax, 3]), what="small")


def test_prefetch_window_long_inputs(dev):
    T, B, V, Lmax = 300, 5, 40, 70
    tg = _labels(3, B, Lmax, V, 0)
    il = np.array([300, 299, 298, 297, 150], dtype=np.int64)
    tl = np.array([70, 64, 33, 10, 70], dtype=np.int64)
    got = _both_passes(dev, _log_probs(3, T, B, V), tg, il, tl, what="T 300")
    assert bool(torch.isfinite(got["nll"]).all())


@pytest.mark.parametrize("blank", [19, 9])
def test_blank_not_zero(dev, blank):
    T, B, V, tg, il, tl = _edge_batch(64, V=20, blank=blank, seed=50)
    _both_passes(dev, _log_probs(blank, T, B, V), tg, il, tl, blank=blank, what="blank %d" % blank)


@pytest.mark.parametrize("zero_infinity", [0, 1])
def test_infeasible_and_bad_lengths(dev, zero_infinity):
    T, B, V, Lmax = 40, 6, 20, 40
    tg = _labels(9, B, Lmax, V, 0)
    il = np.array([T, 20, T + 1, -1, T, T], dtype=np.int64)                  # 1: shorter than its label; 2, 3: outside the tensor
    tl = np.array([10, 30, 5, 5, Lmax + 1, -2], dtype=np.int64)             # 4, 5: outside the tensor
    lp = _log_probs(13, T, B, V)
    got = _both_passes(dev, lp, tg, il, tl, what="lengths", zero_infinity=zero_infinity)
    nll = got["nll"]
    assert bool(torch.isfinite(nll[0])) and bool(torch.isinf(nll[1])) and bool(torch.isnan(nll[2:]).all())
    assert bool(torch.isfinite(got["grad"][:, 0]).all())
    if zero_infinity:
        assert bool((got["grad"][:, 1] == 0).all())


def test_concatenated_targets_through_ctcloss(dev):
    from ctc_pytorch_amd import nn, ops
    T, B, V, Lmax = 90, 6, 30, 40
    tl = np.array([40, 0, 1, 17, 33, 40], dtype=np.int64)
    tg = _labels(17, B, Lmax, V, 0)
    flat = torch.from_numpy(np.concatenate([tg[i, :tl[i]] for i in range(B)])).to(dev)
    il = torch.tensor([90, 50, 3, 88, 89, 87], dtype=torch.int64, device=dev)
    lp = _log_probs(19, T, B, V)
    res = []
    for skew in (0, 1):
        ops.set_option("ctc_lattice_skew", skew)
        try:
            x = lp.to(dev).requires_grad_(True)
            loss = nn.CTCLoss(reduction="mean")(x, flat, il, torch.from_numpy(tl).to(dev))
            loss.backward()
            res.append((loss.detach().cpu().reshape(1), x.grad.cpu()))
        finally:
            ops.set_option("ctc_lattice_skew", 1)
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[1][0]).all())


def test_against_torch_cpu(dev):
    """The skewed kernels held to test_ctc_vs_torch_cpu_random's tolerances (loss 1e-5 relative, gradient 2e-5) on lattices of three waves."""
    from ctc_pytorch_amd import nn, ops
    T, B, V, Lmax = 200, 8, 62, 70
    assert ops.get_option("ctc_lattice_skew") == 1 and ops.ctc_lattice_plan(Lmax)["skewed"] == 1
    rs = np.random.RandomState(23)
    tg = torch.from_numpy(_labels(23, B, Lmax, V, 0))
    tl = torch.from_numpy(rs.randint(10, Lmax + 1, size=B).astype(np.int64))
    tl[0] = Lmax
    il = torch.from_numpy(rs.randint(170, T + 1, size=B).astype(np.int64))
    logits = torch.from_numpy((2 * rs.standard_normal((T, B, V))).astype(np.float32))
    lr = logits.clone().requires_grad_(True)
    loss_r = F.ctc_loss(torch.log_softmax(lr, -1), tg, il, tl, reduction="sum") / B
    loss_r.backward()
    lg = logits.to(dev).requires_grad_(True)
    loss = nn.CTCLoss(reduction="sum")(ops.log_softmax(lg), tg.to(dev), il.to(dev), tl.to(dev)) / B
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_r.detach())) / abs(float(loss_r.detach())) < 1e-5
    assert float((lg.grad.cpu().double() - lr.grad.double()).abs().max()) < 2e-5


@pytest.mark.parametrize("Lmax", [64, 127])
def test_slow_waves_change_nothing(dev, Lmax):
    """Each wave alone, all but the leading one and the leading one only (wave 0 leads the alpha pass, the top wave the beta pass) sleep 32 x 64
    cycles around their ring accesses at every frame -- several frames' worth: the hand-off rests on the barrier and the ring depth."""
    from ctc_pytorch_amd import ops
    W = ops.ctc_lattice_plan(Lmax)["waves"]
    T, B, V = 40, 3, 20
    tg = _labels(29, B, Lmax, V, 0)
    il, tl = np.array([T, T - 1, 9]), np.array([Lmax, Lmax - 1, 3])
    lp = _log_probs(29 + Lmax, T, B, V)
    full = (1 << W) - 1
    masks = sorted({1 << w for w in range(W)} | {full & ~1, full & ~(1 << (W - 1))})
    for with_beta in (True, False):
        ref = _run(dev, lp, tg, il, tl, 0, with_beta, skew=1, slow=0)
        _assert_same(_run(dev, lp, tg, il, tl, 0, with_beta, skew=0), ref, "undelayed")
        for m in masks:
            _assert_same(ref, _run(dev, lp, tg, il, tl, 0, with_beta, skew=1, slow=m), "slow mask %d beta=%s" % (m, with_beta))


def test_two_runs_are_bit_identical(dev):
    T, B, V, tg, il, tl = _edge_batch(127, seed=70)
    lp = _log_probs(31, T, B, V)
    _assert_same(_run(dev, lp, tg, il, tl), _run(dev, lp, tg, il, tl), "rerun")
