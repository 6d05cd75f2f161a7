"""GPU tests of the kernels of lm.hip through the C ABI (include/ctcn.h), against the restatement in tests/lm_ref.py.  Every output lives
inside a NaN-poisoned buffer whose guard words must come back untouched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
IGN = R.IGNORE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _L():
    from ctc_pytorch_amd import _lib
    return _lib.lib(), _lib.stream_ptr()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Out(object):
    """An output of `n` elements of `dtype` inside a poisoned buffer (NaN, or the NaN bit pattern for integers), `shift` elements off the
    buffer's alignment; done() checks the guards and returns the output on the host."""

    def __init__(self, n, dtype, dev, shift=0, fill=None):
        self.poison = float("nan") if dtype.is_floating_point else 0x7FC00000
        self.whole = torch.full((n + 2 * GUARD + shift,), self.poison, dtype=dtype, device=dev)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.t = self.whole[self.lo:self.hi]
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill, dtype=dtype).reshape(-1))

    def done(self):
        w = self.whole.cpu()
        for part in (w[:self.lo], w[self.hi:]):
            ok = torch.isnan(part).all() if w.dtype.is_floating_point else (part == self.poison).all()
            assert bool(ok), "the kernel wrote outside its output"
        return w[self.lo:self.hi].numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


_LIVE = []


@pytest.fixture(autouse=True)
def operands_stay_alive():
    """The C ABI takes raw pointers: every operand uploaded by up() is held until the test is over."""
    yield
    torch.cuda.synchronize()
    del _LIVE[:]


def up(a, dev, shift=0):
    """host array -> device tensor, `shift` elements off the allocation's alignment (kept alive in _LIVE: callers pass its pointer only)"""
    t = torch.as_tensor(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev)
    buf[shift:].copy_(t)
    _LIVE.append(buf)
    return buf[shift:]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 62])
@pytest.mark.parametrize("E", [1, 6, 20, 130])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_embedding_forward_is_a_row_copy(dev, N, E, V):
    """Bit-equal rows for repeated ids, a padding id, a table 4 bytes off its alignment (and an aligned one: the 16-byte path where E allows
    it); one id outside [0, V) gives a row of zeros, raises the status bit and leaves its neighbours correct."""
    L, stream = _L()
    rng = np.random.RandomState(N * 1000 + E * 10 + V)
    table = rng.standard_normal((V, E)).astype(np.float32)
    pad = V - 1
    for shift, bad in ((0, False), (1, False), (0, True)):
        ids = rng.randint(0, V, size=N).astype(np.int32)             # N > V: repeats; `pad` occurs among them for N >= 63
        if N >= 3:
            ids[1] = pad
        if bad:
            ids[N // 2] = V + 3 if N % 2 else -2
        want, want_status = R.embedding_fwd(ids, table, pad)
        y = Out(N * E, torch.float32, dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = L.ctcn_embedding_fwd(P(up(ids, dev)), P(up(table, dev, shift)), P(y.t), N, V, E, pad, P(status), stream)
        assert rc == 0
        got = y.done().reshape(N, E)
        assert np.array_equal(bits(got), bits(want))
        assert int(status.item()) == want_status == (1 if bad else 0)


def _emb_bwd(dev, ids, dy, V, pad, beta, prefill, shift=0):
    L, stream = _L()
    N, E = dy.shape
    out = Out(V * E, torch.float32, dev, shift=shift, fill=prefill)
    nb = L.ctcn_embedding_bwd_ws_bytes(N, V)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    rc = L.ctcn_embedding_bwd(P(up(ids.astype(np.int32), dev)), P(up(dy, dev, shift)), P(out.t), N, V, E, pad, float(beta), P(ws), nb, stream)
    assert rc == 0
    return out.done().reshape(V, E)


EMB_BWD_CASES = {
    "all_equal": (40, 5, 6, lambda rng, N, V: np.full(N, 3)),
    "all_distinct": (37, 37, 20, lambda rng, N, V: rng.permutation(V)),
    "unused_and_padding": (300, 9, 130, lambda rng, N, V: rng.choice([0, 1, 2, 4, 5, 6, 8], size=N)),     # row 3 unused, row 8 = padding, row 7 unused
    "single": (1, 3, 4, lambda rng, N, V: np.array([1])),
    "long_lists": (1000, 3, 12, lambda rng, N, V: rng.randint(0, V, size=N)),
    "two_chunks_odd": (515, 62, 7, lambda rng, N, V: rng.randint(-1, V + 1, size=N)),                     # ids -1 and V: named by nobody
}


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case", sorted(EMB_BWD_CASES))
def test_embedding_backward_equals_the_ascending_loop(dev, case, beta):
    """dtable bit-equal to the float32 loop in ascending n: all ids equal, all distinct, an unused row, the padding row, beta 0 (the
    pre-filled buffer is not read: it holds NaN) and beta 1 on a pre-filled buffer, N = 1, long lists (N = 1000 over V = 3), more than one
    chunk of the counting sort; an unaligned operand pair takes the scalar path to the same bits; two runs give identical bits."""
    N, V, E, make = EMB_BWD_CASES[case]
    rng = np.random.RandomState(len(case) * 7 + N)
    ids = np.asarray(make(rng, N, V))
    pad = 8 if case == "unused_and_padding" else -1
    dy = (rng.standard_normal((N, E)) * np.exp(rng.uniform(-3, 3, size=(N, 1)))).astype(np.float32)
    pre = rng.standard_normal((V, E)).astype(np.float32)
    want = R.embedding_bwd(ids, dy, pre, pad, beta)
    prefill = pre if beta else np.full((V, E), np.nan, dtype=np.float32)
    got = _emb_bwd(dev, ids, dy, V, pad, beta, prefill)
    assert np.array_equal(bits(got), bits(want))
    again = _emb_bwd(dev, ids, dy, V, pad, beta, prefill)
    assert np.array_equal(bits(got), bits(again))
    shifted = _emb_bwd(dev, ids, dy, V, pad, beta, prefill, shift=1)
    assert np.array_equal(bits(shifted), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
def _log_probs(rng, N, V):
    z = (rng.standard_normal((N, V)) * 3).astype(np.float32)
    return torch.log_softmax(torch.from_numpy(z), dim=-1).numpy()


@pytest.mark.parametrize("V", [2, 63, 64, 65, 1000])
@pytest.mark.parametrize("T,B", [(1, 1), (7, 5), (33, 65)])
def test_nll_matches_the_restatement_bit_for_bit(dev, T, B, V):
    """tok, seq_sum, total and count equal to tests/lm_ref.nll on the bits: ignored rows, a column of ignored rows only (sum 0, not NaN),
    a target whose log-prob is -inf (+inf, as torch), and -- in a second call -- a target outside [0, V) (0, status raised)."""
    L, stream = _L()
    rng = np.random.RandomState(T * 100 + B + V)
    N = T * B
    lp = _log_probs(rng, N, V)
    tgt = rng.randint(0, V, size=N).astype(np.int32)
    tgt[rng.rand(N) < 0.2] = IGN
    if B > 1:
        tgt.reshape(T, B)[:, B - 1] = IGN                              # an all-ignored sequence
    if N > 1:
        lp[0, :] = np.float32(-np.log(V - 1)) if V > 1 else 0.0
        tgt[0] = 1 % V
        lp[0, tgt[0]] = -np.inf                                       # a log-softmax row with one impossible class
    for bad in (False, True):
        if bad:
            tgt = tgt.copy()
            tgt[N - 1 if B == 1 else N - 2] = V
        tok_w, seq_w, total_w, count_w, status_w = R.nll(lp, tgt, T, B, IGN)
        tok, sums, count = Out(N, torch.float32, dev), Out(B + 1, torch.float64, dev), Out(1, torch.int32, dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = L.ctcn_nll_fwd(P(up(lp, dev)), P(up(tgt, dev)), T, B, V, IGN, P(tok.t), P(sums.t), P(sums.t[B:]), P(count.t), P(status), stream)
        assert rc == 0
        s = sums.done()
        assert np.array_equal(bits(tok.done()), bits(tok_w))
        assert np.array_equal(bits(s[:B]), bits(seq_w)) and bits(s[B:])[0] == bits(np.array([total_w]))[0]
        assert int(count.done()[0]) == count_w and int(status.item()) == status_w == (2 if bad else 0)
        if B > 1:
            assert s[B - 1] == 0.0
        if N > 1:
            assert tok_w[0] == np.inf and s[0] == np.inf


def _xent_rows(rng, N, V):
    """log-prob rows and targets of the cases the issue lists: peaked on the target, peaked on another class, uniform, -inf entries, random;
    some rows ignored.  The rows are proper log-softmax outputs (float32)."""
    z = np.zeros((N, V), dtype=np.float32)
    tgt = rng.randint(0, V, size=N).astype(np.int32)
    for n in range(N):
        kind = n % 5
        if kind == 0:                                   # target at 0, the others at -80
            z[n] = -80.0
            z[n, tgt[n]] = 0.0
        elif kind == 1:                                 # the wrong class peaked
            z[n] = -80.0
            z[n, (tgt[n] + 1) % V] = 0.0
        elif kind == 2:
            z[n] = 0.0
        elif kind == 3:
            z[n] = rng.standard_normal(V) * 2
            z[n, rng.rand(V) < 0.3] = -np.inf
            z[n, (tgt[n] + 1) % V] = 1.0                # (never a row of -inf only)
        else:
            z[n] = rng.standard_normal(V) * 4
    lp = torch.log_softmax(torch.from_numpy(z), dim=-1).numpy()
    tgt[rng.rand(N) < 0.15] = IGN
    if N > 2:
        tgt[2] = IGN
    return lp, tgt


@pytest.mark.parametrize("mode", ["none", "sum", "mean"])
@pytest.mark.parametrize("V", [2, 63, 64, 65, 512, 516, 1000, 8192])
def test_xent_backward_is_within_the_derived_bound(dev, V, mode):
    """dz against float64 on the same float32 lp bits, element by element under tests/lm_ref.xent_bound (derivation there: expf 1 ulp, one
    subtraction, one product, the 'mean' division, times |g_n|) -- no tolerance found by trial.  Stride-1 g ('none'), stride-0 g ('sum'),
    'mean' through the device count; V on both sides of the wave-per-row / workgroup-per-row switch (512 | 516) and both the 16-byte path
    (V % 4 == 0) and the scalar one; ignored rows and out-of-range rows are exact zeros; -inf log-probs give probability 0, never NaN."""
    L, stream = _L()
    N = 23 if V < 8192 else 9
    rng = np.random.RandomState(V + len(mode))
    lp, tgt = _xent_rows(rng, N, V)
    if mode == "none":
        g, stride = (rng.standard_normal(N) * 3).astype(np.float32), 1
    else:
        g, stride = np.array([1.7], dtype=np.float32), 0
    cnt = int((tgt != IGN).sum())
    count = torch.tensor([cnt], dtype=torch.int32, device=dev) if mode == "mean" else None
    want, p, y, gn = R.xent_bwd(lp, tgt, g, stride, cnt if mode == "mean" else None, IGN)
    bound = R.xent_bound(p, y, gn, mode == "mean")
    for shift in (0, 1):
        dz = Out(N * V, torch.float32, dev, shift=shift)
        rc = L.ctcn_xent_bwd(P(up(lp, dev, shift)), P(up(tgt, dev)), P(dz.t), N, V, IGN, P(up(g, dev)), stride, P(count), stream)
        assert rc == 0
        got = dz.done().reshape(N, V).astype(np.float64)
        assert np.isfinite(got).all()
        dead = tgt == IGN
        assert not got[dead].any()
        err = np.abs(got - want)
        frac = float((err / bound).max())
        print("xent_bwd V=%d %s shift=%d: max error / bound = %.3f" % (V, mode, shift, frac))
        assert (err <= bound).all(), frac


def test_xent_backward_zeroes_a_row_whose_target_is_out_of_range(dev):
    L, stream = _L()
    rng = np.random.RandomState(5)
    lp = _log_probs(rng, 4, 7)
    tgt = np.array([1, 7, -3, 2], dtype=np.int32)
    g = np.ones(1, dtype=np.float32)
    dz = Out(28, torch.float32, dev)
    assert L.ctcn_xent_bwd(P(up(lp, dev)), P(up(tgt, dev)), P(dz.t), 4, 7, IGN, P(up(g, dev)), 0, None, stream) == 0
    got = dz.done().reshape(4, 7)
    assert not got[1].any() and not got[2].any() and got[0].any() and got[3].any()


# ---------------------------------------------------------------------------------------------------------------------------------
def _nbest(rng, B, N, T):
    out_ids = rng.randint(1, 12, size=(B, N, T)).astype(np.int32)
    out_len = rng.randint(0, T + 1, size=(B, N)).astype(np.int32)
    out_len[0, 0] = 0                                                   # a zero-length hypothesis
    out_len[B - 1, N - 1] = T
    count = np.array([min(b, N) for b in range(B)], dtype=np.int32)     # 0 .. N
    count[B - 1] = N
    score = -rng.rand(B, N) * 10
    lm = -rng.rand(B, N) * 30
    return out_ids, out_len, count, score, lm


@pytest.mark.parametrize("N", [1, 4])
def test_pack_and_select_equal_the_restatement(dev, N):
    """B = 5, T = 9, counts from 0 to N, zero-length hypotheses, exact ties between totals (the lowest k wins): every integer equal, every
    float64 bit-equal; L below the longest labelling clamps; weight 0 and bonus 0 give entry 0 with its own score."""
    L, stream = _L()
    B, T = 5, 9
    rng = np.random.RandomState(40 + N)
    out_ids, out_len, count, score, lm = _nbest(rng, B, N, T)
    if N > 1:                                                           # exact ties: equal score, equal lm, equal length
        score[B - 1, 1], lm[B - 1, 1], out_len[B - 1, 1] = score[B - 1, 2], lm[B - 1, 2], out_len[B - 1, 2]
        score[B - 1, 1:3], lm[B - 1, 1:3] = 100.0, 0.0                  # ... and they are the best under every weight below
    d = lambda a: up(a, dev)
    for Lmax in (int(out_len.max()), 4):
        S = B * N
        ids_o, tgt_o, lens_o = (Out((Lmax + 1) * S, torch.int32, dev), Out((Lmax + 1) * S, torch.int32, dev), Out(S, torch.int32, dev))
        rc = L.ctcn_lm_pack_nbest(P(d(out_ids)), P(d(out_len)), P(d(count)), B, N, T, Lmax, R.BOUNDARY, IGN, P(ids_o.t), P(tgt_o.t), P(lens_o.t), stream)
        assert rc == 0
        wi, wt, wl = R.pack_nbest(out_ids, out_len, count, Lmax)
        assert np.array_equal(ids_o.done().reshape(Lmax + 1, S), wi) and np.array_equal(tgt_o.done().reshape(Lmax + 1, S), wt)
        assert np.array_equal(lens_o.done(), wl) and wl.min() >= 1
    for weight, bonus in ((0.5, 0.0), (0.3, 0.7), (0.0, 0.0), (1e6, -0.25)):
        bi, bl, bs, bk = Out(B * T, torch.int32, dev), Out(B, torch.int32, dev), Out(B, torch.float64, dev), Out(B, torch.int32, dev)
        rc = L.ctcn_rescore_select(P(d(score)), P(d(lm)), P(d(out_len)), P(d(count)), P(d(out_ids)), weight, bonus, B, N, T, P(bi.t), P(bl.t),
                                   P(bs.t), P(bk.t), stream)
        assert rc == 0
        wi, wl, ws, wk = R.rescore_select(score, lm, out_len, count, out_ids, weight, bonus)
        assert np.array_equal(bi.done().reshape(B, T), wi) and np.array_equal(bl.done(), wl) and np.array_equal(bk.done(), wk)
        assert np.array_equal(bits(bs.done()), bits(ws))
        assert wk[0] == -1 and wl[0] == 0
        if N > 1:
            assert wk[B - 1] == 1                                       # the tie goes to the lower k
        if weight == 0.0 and bonus == 0.0:
            live = count > 0
            assert np.array_equal(bits(ws[live]), bits(np.array([score[b, wk[b]] for b in range(B) if live[b]])))
