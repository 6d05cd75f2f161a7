"""CTC forced alignment on the HIP kernel (ctcn_ctc_align through ops.ctc_forced_align / Decoder.align) against the float32 numpy
restatement of tests/test_ctc_align_host.py: the recursion is a max and one rounded add with a fixed tie rule, so scores are compared on
their bits and paths / spans with ==.  Both homes of the back-pointer rows are exercised: LDS (every ordinary shape) and the workspace
(long labels, and a long input with a short label)."""
import numpy as np
import pytest
import torch

from ctc_pytorch_amd.testing import synth
from test_ctc_align_host import align_ref
from test_ctc_loss_modes import _ragged_batch

pytestmark = pytest.mark.gpu

FIELDS = ("paths", "frame_scores", "scores", "ok", "starts", "ends")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _host(out):
    return {k: getattr(out, k).cpu().numpy() for k in FIELDS}


def _log_softmax(z):
    z = z.astype(np.float64)
    m = z.max(axis=-1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))).astype(np.float32)


def _labels(rs, B, Lmax, V, blank, tl):
    lab = rs.randint(0, V - 1, size=(B, Lmax))
    lab = lab + (lab >= blank)                                    # every class but the blank
    tg = np.zeros((B, Lmax), dtype=np.int64)
    for i in range(B):
        tg[i, :tl[i]] = lab[i, :tl[i]]
    return tg


def _check(dev, lp, tg, il, tl, blank, expect_ws=None):
    """Run the kernel on (lp, padded targets, lengths), compare every output with the restatement; returns (ours, reference) on the host."""
    from ctc_pytorch_amd import _lib, ops
    T, B, _ = lp.shape
    need = _lib.lib().ctcn_ctc_align_ws_bytes(T, B, tg.shape[1])
    if expect_ws is not None:
        assert (need > 0) == expect_ws, need
    out = ops.ctc_forced_align(torch.from_numpy(lp).to(dev), torch.from_numpy(tg).to(dev), torch.from_numpy(np.asarray(il, dtype=np.int64)).to(dev),
                               torch.from_numpy(np.asarray(tl, dtype=np.int64)).to(dev), blank=blank)
    got, ref = _host(out), align_ref(lp, tg, il, tl, blank)
    for k in FIELDS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape, ref[k].shape)
        same = _bits(got[k]) == _bits(ref[k])
        assert same.all(), (k, np.argwhere(~same)[:5].tolist(), got[k][~same][:5], ref[k][~same][:5])
    # frame_scores are the log-probs along the path
    for b in range(B):
        n = int(il[b]) if got["ok"][b] else 0
        p = got["paths"][b, :n]
        assert np.array_equal(_bits(got["frame_scores"][b, :n]), _bits(lp[np.arange(n), b, p]))
        feasible_spans = got["ok"][b] and int(tl[b]) > 0
        if feasible_spans:
            s, e = got["starts"][b, :tl[b]], got["ends"][b, :tl[b]]
            assert (s < e).all() and (s[1:] >= e[:-1]).all() and s[0] >= 0 and e[-1] <= il[b]
    return got, ref


def test_align_cfg2_shape_ragged_batch(dev):
    """synth's ragged batch at cfg2's shape (T = 800, B = 32, V = 62), peaky and flat posteriors."""
    T, B, V = 800, 32, 62
    b = synth.make_batch(seed=11, B=B, T=T, F=4, V=V, lab_lo=30, lab_hi=60)
    for regime in ("peaky", "flat"):
        lp = synth.make_logprobs(21, T, B, V, regime)
        got, _ = _check(dev, lp, b["targets"], b["lens"], b["tgt_len"], 0, expect_ws=False)
        assert got["ok"].all()


@pytest.mark.parametrize("blank", [0, 5, 61])
def test_align_hand_set_rows(dev, blank):
    """The rows of the loss tests' ragged batch: empty label (0), infeasible (1, 3), a long run of repeats (2), a short input (4)."""
    logits, tg, il, tl = _ragged_batch(blank)
    got, _ = _check(dev, _log_softmax(logits), tg, il, tl, blank, expect_ws=False)
    assert got["ok"][[1, 3]].tolist() == [0, 0] and np.isneginf(got["scores"][[1, 3]]).all()
    assert got["ok"][[0, 2, 4]].tolist() == [1, 1, 1]
    assert (got["paths"][0, :il[0]] == blank).all() and (got["starts"][0] == -1).all()
    assert (got["paths"][1] == -1).all() and (got["frame_scores"][1] == 0).all() and (got["starts"][1] == -1).all() and (got["ends"][1] == -1).all()
    assert (got["paths"][4, il[4]:] == -1).all() and (got["frame_scores"][4, il[4]:] == 0).all()
    assert (got["starts"][4, tl[4]:] == -1).all() and (got["ends"][4, tl[4]:] == -1).all()


@pytest.mark.parametrize("V", [2, 62, 4097])
def test_align_vocabulary_sizes(dev, V):
    T, B = 96, 5
    rs = np.random.RandomState(V)
    for blank in sorted({0, min(5, V - 1), V - 1}):
        tl = np.array([0, 1, 7, 20, 40])
        tg = _labels(rs, B, 40, V, blank, tl)
        il = np.array([T, 3, 50, T, 60])
        lp = _log_softmax(2 * rs.standard_normal((T, B, V)))
        _check(dev, lp, tg, il, tl, blank)


def test_align_long_labels_run_sixteen_states_per_thread_and_the_workspace(dev):
    """L = 2047 (S = 4095: sixteen states per thread, 256 words per back-pointer row): the rows go to the workspace and come back in chunks
    of 8 frames.  T is large enough for the repeats the random labels contain."""
    T, B, V = 2400, 2, 40
    rs = np.random.RandomState(3)
    tl = np.array([2047, 1500])
    tg = _labels(rs, B, 2047, V, V - 1, tl)
    il = np.array([T, 2000])
    lp = _log_softmax(1.5 * rs.standard_normal((T, B, V)))
    got, _ = _check(dev, lp, tg, il, tl, V - 1, expect_ws=True)
    assert got["ok"].tolist() == [1, 1]


def test_align_long_input_short_label_takes_the_workspace(dev):
    """T = 20 000 frames with up to 5 labels: one word per row, but 80 KB of rows -- the workspace branch with 1 024-frame chunks, one
    state per thread; also an infeasible and an empty row on that branch."""
    T, B, V = 20000, 4, 8
    rs = np.random.RandomState(8)
    tl = np.array([5, 3, 0, 4])
    tg = _labels(rs, B, 5, V, 2, tl)
    tg[3, :4] = tg[3, 0]
    il = np.array([T, 12345, 700, 6])                         # row 3: four repeats need 7 frames
    lp = _log_softmax(2 * rs.standard_normal((T, B, V)))
    got, _ = _check(dev, lp, tg, il, tl, 2, expect_ws=True)
    assert got["ok"].tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("Lmax", [100, 200, 300, 700, 1200])
def test_align_states_per_thread(dev, Lmax):
    """S = 201 / 401 / 601 / 1401 / 2401: 1, 2, 4, 8 and 16 states per thread; the first two keep their rows in LDS, the others (T = 2 Lmax + 40
    frames of 38 ... 151 words) use the workspace."""
    T, B, V = 2 * Lmax + 40, 3, 30
    rs = np.random.RandomState(Lmax)
    tl = np.array([Lmax, Lmax // 2, 130 if Lmax > 130 else 17])
    tg = _labels(rs, B, Lmax, V, 7, tl)
    il = np.array([T, T - 11, T // 2])
    lp = _log_softmax(2 * rs.standard_normal((T, B, V)))
    got, _ = _check(dev, lp, tg, il, tl, 7, expect_ws=Lmax > 200)
    assert got["ok"].all()


def test_align_ties_and_minus_infinity(dev):
    """Log-probs quantised to multiples of 0.5 (ties on most frames) and rows that contain -inf (classes that cannot be emitted)."""
    T, B, V = 300, 8, 12
    rs = np.random.RandomState(17)
    tl = rs.randint(5, 60, size=B)
    tg = _labels(rs, B, int(tl.max()), V, 3, tl)
    il = rs.randint(150, T + 1, size=B)
    lp = (np.round(2 * _log_softmax(rs.standard_normal((T, B, V)))) / 2).astype(np.float32)
    got, _ = _check(dev, lp, tg, il, tl, 3)
    assert got["ok"].all()
    lp = np.round(rs.randint(-2, 1, size=(T, B, V))).astype(np.float32)                 # three values: ties nearly everywhere
    _check(dev, lp, tg, il, tl, 3)
    lp = _log_softmax(2 * rs.standard_normal((T, B, V)))
    lp[rs.random_sample((T, B, V)) < 0.05] = -np.inf
    lp[:, 0, 3] = -np.inf                                                                 # utterance 0 can never emit the blank
    lp[:, 1, tg[1, 0]] = -np.inf                                                          # utterance 1 can never emit its first label
    got, _ = _check(dev, lp, tg, il, tl, 3)
    assert got["ok"][1] == 0 and 0 < got["ok"].sum() < B


def test_align_empty_targets_and_edge_lengths(dev):
    """Lmax = 0 (every target empty), Tb = 0 / 1, lengths outside the tensors (device lengths: the kernel answers NaN)."""
    T, B, V = 50, 4, 6
    rs = np.random.RandomState(2)
    lp = _log_softmax(rs.standard_normal((T, B, V)))
    got, _ = _check(dev, lp, np.zeros((B, 0), np.int64), np.array([T, 0, 1, 20]), np.zeros(B, np.int64), 4, expect_ws=False)
    assert got["ok"].all() and got["starts"].shape == (B, 0) and (got["paths"][0] == 4).all() and got["scores"][1] == 0
    tl = np.array([1, 1, 3, 2])
    tg = _labels(rs, B, 3, V, 0, np.array([3, 3, 3, 3]))
    got, _ = _check(dev, lp, tg, np.array([1, 0, T + 1, -1]), tl, 0)
    assert got["ok"].tolist() == [1, 0, 0, 0] and np.isneginf(got["scores"][1]) and np.isnan(got["scores"][2:]).all()
    got, _ = _check(dev, lp, tg, np.array([T, T, T, T]), np.array([3, 4, -1, 0]), 0)
    assert got["ok"].tolist() == [1, 0, 0, 1] and np.isnan(got["scores"][1:3]).all()


def test_align_structure_against_greedy_collapse_and_the_loss(dev):
    """Without the restatement: the path collapses to the target; the best path never beats the sum over paths (score <= -nll up to the
    loss test's 1e-5 relative slack of the float32 log-sum-exp); an alignment exists exactly where the loss is finite."""
    from ctc_pytorch_amd import ops
    for blank in (0, 61):
        logits, tg, il, tl = _ragged_batch(blank)
        lp = ops.log_softmax(torch.from_numpy(logits).to(dev))
        args = (torch.from_numpy(tg).to(dev), torch.from_numpy(il).to(dev), torch.from_numpy(tl).to(dev))
        out = ops.ctc_forced_align(lp, *args, blank=blank)
        nll = ops.ctc_loss(lp, *args, blank=blank, reduction="none").cpu().numpy().astype(np.float64)
        ok, sc = out.ok.cpu().numpy(), out.scores.cpu().numpy().astype(np.float64)
        assert np.array_equal(ok != 0, np.isfinite(nll))
        fin = ok != 0
        assert (sc[fin] <= -nll[fin] + 1e-5 * np.abs(nll[fin])).all(), (sc[fin] + nll[fin]).max()
        paths = out.paths.clone()
        paths[paths < 0] = blank
        ids, n = ops.greedy_collapse(paths, args[1].to(torch.int32), blank=blank, batch_major=True)
        ids, n = ids.cpu().numpy(), n.cpu().numpy()
        for b in np.nonzero(fin)[0]:
            assert n[b] == tl[b] and ids[b, :n[b]].tolist() == tg[b, :tl[b]].tolist(), b


def test_align_recovers_a_known_alignment(dev):
    """One-hot-like posteriors built from a known state sequence: that sequence comes back, spans included."""
    T, B, V, blank = 120, 6, 20, 0
    rs = np.random.RandomState(4)
    lp = np.full((T, B, V), np.log(0.01 / (V - 1)), dtype=np.float32)
    tl = np.array([1, 4, 9, 15, 0, 30])
    Lmax = int(tl.max())
    tg = np.zeros((B, Lmax), dtype=np.int64)
    il = np.array([T, 100, 77, T, 40, 61])
    want_paths = np.full((B, T), -1, dtype=np.int32)
    want_s, want_e = np.full((B, Lmax), -1, np.int32), np.full((B, Lmax), -1, np.int32)
    for b in range(B):
        t = 0
        for j in range(tl[b]):
            c = int(rs.randint(1, V))
            tg[b, j] = c
            room = il[b] - t - 2 * (tl[b] - j)                    # frames that may be spent here and still fit the rest with its blanks
            gap = int(rs.randint(1, max(2, min(4, room)))) if (j > 0 and tg[b, j - 1] == c) else int(rs.randint(0, max(1, min(3, room))))
            want_paths[b, t:t + gap] = blank
            t += gap
            run = int(rs.randint(1, max(2, min(4, room - gap + 1))))
            want_paths[b, t:t + run] = c
            want_s[b, j], want_e[b, j] = t, t + run
            t += run
        assert t <= il[b]
        want_paths[b, t:il[b]] = blank
        lp[np.arange(il[b]), b, want_paths[b, :il[b]]] = np.float32(np.log(0.99))
    got, _ = _check(dev, lp, tg, il, tl, blank)
    assert got["ok"].all()
    assert np.array_equal(got["paths"], want_paths) and np.array_equal(got["starts"], want_s) and np.array_equal(got["ends"], want_e)


@pytest.mark.parametrize("lengths_on", ["host", "device"])
def test_align_target_layouts_length_types_and_unbatched(dev, lengths_on):
    from ctc_pytorch_amd import ops
    logits, tg, il, tl = _ragged_batch(blank=1)
    il = np.minimum(il, logits.shape[0])
    feasible = [0, 2, 4, 5, 6, 7]                                 # host lengths are validated on the host: keep them inside the tensors
    logits, tg, il, tl = logits[:, feasible], tg[feasible], il[feasible], tl[feasible]
    B = len(feasible)
    flat = torch.from_numpy(np.concatenate([tg[i, :tl[i]] for i in range(B)]))
    lp = ops.log_softmax(torch.from_numpy(logits).to(dev))
    padded = ops.ctc_forced_align(lp, torch.from_numpy(tg).to(dev), torch.from_numpy(il).to(dev), torch.from_numpy(tl).to(dev), blank=1)
    ilx, tlx = (torch.from_numpy(il).to(dev), torch.from_numpy(tl).to(dev)) if lengths_on == "device" else (il.tolist(), tuple(tl.tolist()))
    conc = ops.ctc_forced_align(lp, flat if lengths_on == "host" else flat.to(dev), ilx, tlx, blank=1)
    Lc = int(tl.max())
    for k in FIELDS:
        a, c = getattr(padded, k).cpu(), getattr(conc, k).cpu()
        if k in ("starts", "ends"):                               # concatenated targets: Lmax = max(target_lengths)
            assert bool((a[:, Lc:] == -1).all())
            a = a[:, :Lc]
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), k
    for b in (0, 1, 3):                                           # unbatched (T, C): a batch of one, the batch dimension dropped
        n = int(tl[b])
        one = ops.ctc_forced_align(lp[:, b], torch.from_numpy(tg[b, :n]).to(dev), int(il[b]) if lengths_on == "host" else torch.tensor(il[b]).to(dev),
                                   n if lengths_on == "host" else torch.tensor(n).to(dev), blank=1)
        assert one.paths.shape == (lp.shape[0],) and one.scores.shape == () and one.ok.shape == () and one.starts.shape == (n,)
        for k in FIELDS:
            a, c = getattr(padded, k)[b].cpu(), getattr(one, k).cpu()
            a = a[:n] if k in ("starts", "ends") else a
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (b, k)


@pytest.mark.parametrize("shape", ["lds", "workspace"])
def test_align_writes_every_output_element(dev, shape):
    """Through the C ABI with every output pre-filled with a sentinel: none survives, on either branch, for feasible, infeasible, empty,
    short and out-of-range utterances."""
    import ctypes
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    T, B, V, Lmax = (200, 6, 9, 25) if shape == "lds" else (9000, 6, 9, 25)
    rs = np.random.RandomState(6)
    tl = np.array([25, 10, 0, 25, 3, 30])
    tg = _labels(rs, B, Lmax, V, 8, np.minimum(tl, Lmax))
    il = np.array([T, T // 2, T // 3, 20, 0, T])                 # row 3 infeasible, row 4 without frames, row 5 label length out of range
    lp = _log_softmax(rs.standard_normal((T, B, V)))
    need = L.ctcn_ctc_align_ws_bytes(T, B, Lmax)
    assert (need > 0) == (shape == "workspace")
    d = lambda a: torch.from_numpy(a).to(dev)
    lp_d, tg_d, il_d, tl_d = d(lp), d(tg), d(il.astype(np.int64)), d(tl.astype(np.int64))
    SI, SF = -77, -12345.5
    paths = torch.full((B, T), SI, dtype=torch.int32, device=dev)
    fs = torch.full((B, T), SF, dtype=torch.float32, device=dev)
    sc = torch.full((B,), SF, dtype=torch.float32, device=dev)
    ok = torch.full((B,), SI, dtype=torch.int32, device=dev)
    st = torch.full((B, Lmax), SI, dtype=torch.int32, device=dev)
    en = torch.full((B, Lmax), SI, dtype=torch.int32, device=dev)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.ctcn_ctc_align(p(lp_d), p(tg_d), p(il_d), p(tl_d), p(paths), p(fs), p(sc), p(ok), p(st), p(en), T, B, V, Lmax, 8,
                          p(ws) if need else None, need, _lib.stream_ptr())
    assert rc == 0, L.ctcn_last_error()
    torch.cuda.synchronize()
    for t, s in ((paths, SI), (fs, SF), (sc, SF), (ok, SI), (st, SI), (en, SI)):
        assert not bool((t == s).any())
    ref = align_ref(lp, tg, il, tl, 8)
    for k, t in zip(FIELDS, (paths, fs, sc, ok, st, en)):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(ref[k])), k
    assert ok.cpu().tolist() == [1, 1, 1, 0, 0, 0]
    # starts / ends are optional
    paths2 = torch.full_like(paths, SI)
    rc = L.ctcn_ctc_align(p(lp_d), p(tg_d), p(il_d), p(tl_d), p(paths2), p(fs), p(sc), p(ok), None, None, T, B, V, Lmax, 8,
                          p(ws) if need else None, need, _lib.stream_ptr())
    assert rc == 0 and torch.equal(paths2, paths)


def test_decoder_align_tokens_spans_and_means(dev, tmp_path):
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder, GreedyDecoder
    T, B, V = 60, 4, 62
    b = synth.make_batch(seed=5, B=B, T=T, F=4, V=V, lab_lo=3, lab_hi=9)
    tl, il = b["tgt_len"].copy(), b["lens"].copy()
    tl[2], il[2] = 3, 2                                          # no alignment: more labels than frames
    tg = b["targets"]
    lp = synth.make_logprobs(9, T, B, V, "flat")
    flat = np.concatenate([tg[i, :tl[i]] for i in range(B)])
    names = synth.int2char(V)
    ref = align_ref(lp, tg, il, tl, 0)
    arpa = str(tmp_path / "lm.arpa")
    synth.write_arpa(arpa, [names[i] for i in range(1, V)], seed=3, n_bigrams=40)
    for dec in (GreedyDecoder(names, space_idx=-1, blank_index=0), BeamDecoder(names, beam_width=5, blank_index=0, space_idx=-1, lm_path=arpa)):
        for stride in (1, 4):
            res = dec.align(torch.from_numpy(lp).to(dev), il.tolist(), torch.from_numpy(flat), tl.tolist(), frame_stride=stride)
            assert len(res) == B and res[2] is None
            for i in (0, 1, 3):
                spans, score = res[i]
                assert np.float32(score) == ref["scores"][i] and len(spans) == tl[i]
                for j, (tok, s, e, mean) in enumerate(spans):
                    rs_, re_ = int(ref["starts"][i, j]), int(ref["ends"][i, j])
                    assert tok == names[int(tg[i, j])] and (s, e) == (rs_ * stride, re_ * stride)
                    want = float(np.mean(ref["frame_scores"][i, rs_:re_].astype(np.float64)))
                    assert abs(mean - want) <= 1e-12 * max(1.0, abs(want)) * T, (mean, want)


def test_align_is_a_function_of_its_input(dev):
    """Two consecutive calls and a call on a non-default stream give identical bits (no learnt state), on both branches."""
    from ctc_pytorch_amd import ops
    for T, B, V, lo, hi in ((400, 8, 30, 10, 50), (9000, 3, 30, 10, 50)):
        b = synth.make_batch(seed=T, B=B, T=T, F=4, V=V, lab_lo=lo, lab_hi=hi)
        lp = torch.from_numpy((np.round(4 * synth.make_logprobs(3, T, B, V, "flat")) / 4).astype(np.float32)).to(dev)
        args = (torch.from_numpy(b["targets"]).to(dev), torch.from_numpy(b["lens"]).to(dev), torch.from_numpy(b["tgt_len"]).to(dev))
        first = ops.ctc_forced_align(lp, *args)
        second = ops.ctc_forced_align(lp, *args)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            third = ops.ctc_forced_align(lp, *args)
        side.synchronize()
        for k in FIELDS:
            a = getattr(first, k).view(torch.int32)
            assert torch.equal(a, getattr(second, k).view(torch.int32)) and torch.equal(a, getattr(third, k).view(torch.int32)), k
        assert bool(first.ok.all())
