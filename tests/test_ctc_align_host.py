"""CTC forced alignment, the part that runs without a GPU: the float32 numpy restatement of the definition (include/ctcn.h,
ctcn_ctc_align) that tests/test_ctc_align.py compares the kernel with bit for bit, checked here against exhaustive enumeration of all
V^T paths and a float64 Viterbi pass; the argument errors ops.ctc_forced_align and the C ABI raise before any device work; the host
half of Decoder.align."""
import itertools
import os

import numpy as np
import pytest
import torch

NEG = np.float32(-np.inf)


# ---------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------
def _extended(target, blank):
    L = len(target)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(target, dtype=np.int64)
    skip = np.zeros(2 * L + 1, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]           # s odd, s >= 2 (so s >= 3), ext(s) != ext(s - 2)
    return ext, skip


def viterbi(lp, target, blank, dtype=np.float32):
    """One utterance: lp (Tb, V), Tb >= 1.  v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if allowed) + lp[t, ext(s)], one add of
    `dtype` per cell; ties to the smallest move (a candidate replaces the best so far only if strictly greater); end state S-1, or S-2
    only if strictly greater.  Returns (score, states) -- states None when the score is -inf."""
    lp = np.asarray(lp, dtype=dtype)
    Tb = lp.shape[0]
    ext, skip = _extended(target, blank)
    S = len(ext)
    ninf = dtype(-np.inf)
    v = np.full(S, ninf, dtype=dtype)
    v[:2] = lp[0, ext[:2]]
    moves = np.zeros((Tb, S), dtype=np.int8)
    for t in range(1, Tb):
        x1 = np.concatenate([[ninf], v[:-1]]).astype(dtype)
        x2 = np.where(skip, np.concatenate([[ninf, ninf], v[:-2]])[:S], ninf).astype(dtype)
        best, code = v.copy(), np.zeros(S, dtype=np.int8)
        m = x1 > best
        best[m], code[m] = x1[m], 1
        m = x2 > best
        best[m], code[m] = x2[m], 2
        with np.errstate(invalid="ignore"):
            v = (best + lp[t, ext]).astype(dtype)
        moves[t] = code
    s = S - 2 if S > 1 and v[S - 2] > v[S - 1] else S - 1
    score = v[s]
    if score == ninf:
        return score, None
    states = np.empty(Tb, dtype=np.int64)
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(moves[t, s])
    return score, states


def align_ref(lp, targets, in_len, tgt_len, blank):
    """The outputs of ctcn_ctc_align for a batch: lp (T, B, V) float32, targets (B, Lmax) padded."""
    lp = np.asarray(lp, dtype=np.float32)
    T, B, _ = lp.shape
    Lmax = targets.shape[1] if B else 0
    out = dict(paths=np.full((B, T), -1, np.int32), frame_scores=np.zeros((B, T), np.float32), scores=np.zeros(B, np.float32),
               ok=np.zeros(B, np.int32), starts=np.full((B, Lmax), -1, np.int32), ends=np.full((B, Lmax), -1, np.int32))
    for b in range(B):
        Tb, L = int(in_len[b]), int(tgt_len[b])
        if Tb < 0 or Tb > T or L < 0 or L > Lmax:
            out["scores"][b] = np.nan
            continue
        if Tb == 0:
            out["ok"][b], out["scores"][b] = int(L == 0), 0.0 if L == 0 else NEG
            continue
        score, states = viterbi(lp[:Tb, b], targets[b, :L], blank)
        out["scores"][b] = score
        if states is None:
            continue
        ext, _ = _extended(targets[b, :L], blank)
        out["ok"][b] = 1
        out["paths"][b, :Tb] = ext[states]
        out["frame_scores"][b, :Tb] = lp[np.arange(Tb), b, ext[states]]
        for j in range(L):
            at = np.nonzero(states == 2 * j + 1)[0]
            out["starts"][b, j], out["ends"][b, j] = at[0], at[-1] + 1
    return out


def collapse(path, blank):
    return [int(c) for i, c in enumerate(path) if c != blank and (i == 0 or c != path[i - 1])]


def slack(lp):
    """Float32 DP against a float64 optimum: each of the Tb adds rounds once, relative to a partial sum bounded by sum_t max_c |lp[t, c]|;
    factor 2 for comparing two paths."""
    lp = np.asarray(lp, dtype=np.float64)
    fin = np.where(np.isfinite(lp), np.abs(lp), 0.0)
    return 2.0 * lp.shape[0] * 2.0 ** -24 * float(fin.max(axis=1).sum())


# ---------------------------------------------------------------------------------------------------------
# the restatement against enumeration and float64
# ---------------------------------------------------------------------------------------------------------
def _tiny_cases(n=300, seed=1234):
    rs = np.random.RandomState(seed)
    for i in range(n):
        T, V = int(rs.randint(1, 7)), int(rs.randint(2, 5))
        L = int(rs.randint(0, min(3, T) + 1))
        blank = int(rs.randint(0, V))
        classes = [c for c in range(V) if c != blank]
        target = [int(classes[k]) for k in rs.randint(0, len(classes), size=L)]
        if i % 3 == 0:
            lp = rs.randint(-3, 1, size=(T, V)).astype(np.float32)          # small integers: ties everywhere, sums exact
        else:
            z = rs.standard_normal((T, V)) * 2
            lp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
        yield i % 3 == 0, lp, target, blank


def test_restatement_is_optimal_against_exhaustive_enumeration():
    feasible = 0
    total = 0
    for exact, lp, target, blank in _tiny_cases():
        total += 1
        T, V = lp.shape
        best = None
        for path in itertools.product(range(V), repeat=T):
            if collapse(path, blank) == target:
                sc = float(np.sum(lp[np.arange(T), list(path)], dtype=np.float64))
                best = sc if best is None or sc > best else best
        score, states = viterbi(lp, target, blank)
        if best is None:
            assert states is None and score == NEG
            continue
        feasible += 1
        assert states is not None
        ext, _ = _extended(target, blank)
        path = ext[states]
        assert collapse(path, blank) == target
        assert states[0] <= 1 and states[-1] >= len(ext) - 2 and np.all(np.diff(states) >= 0) and np.all(np.diff(states) <= 2)
        along = float(np.sum(lp[np.arange(T), path], dtype=np.float64))
        if exact:
            assert along == best and float(score) == best
        else:
            assert best - along <= slack(lp) and abs(float(score) - best) <= slack(lp)
    assert total == 300 and feasible >= total // 2, (feasible, total)


def test_restatement_score_is_within_rounding_of_a_float64_viterbi():
    rs = np.random.RandomState(5)
    for T, V, L in ((40, 20, 12), (200, 62, 50), (64, 5, 30)):
        blank = int(rs.randint(0, V))
        target = [int(c) for c in rs.randint(0, V - 1, size=L)]
        target = [c + (c >= blank) for c in target]
        z = 2 * rs.standard_normal((T, V))
        lp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
        s32, st32 = viterbi(lp, target, blank)
        s64, st64 = viterbi(lp, target, blank, dtype=np.float64)
        assert st64 is not None and st32 is not None
        assert abs(float(s32) - float(s64)) <= slack(lp), (float(s32), float(s64), slack(lp))
        ext, _ = _extended(target, blank)
        along = float(np.sum(lp[np.arange(T), ext[st32]], dtype=np.float64))
        assert float(s64) - along <= slack(lp)


def test_ties_go_to_the_smallest_move():
    # all-equal log-probs: the label is entered at frame 0 and left as early as possible, the rest is the trailing blank
    lp = np.zeros((3, 3), dtype=np.float32)
    score, states = viterbi(lp, [1], blank=0)
    assert float(score) == 0.0 and states.tolist() == [1, 2, 2]
    out = align_ref(lp[:, None, :], np.array([[1]]), [3], [1], 0)
    assert out["paths"].tolist() == [[1, 0, 0]] and out["starts"].tolist() == [[0]] and out["ends"].tolist() == [[1]]
    # the end state is S-2 only when strictly greater
    lp = np.array([[0, 0], [0, -1]], dtype=np.float32)            # blank 1: ending on the blank costs 1
    score, states = viterbi(lp, [0], blank=1)
    assert float(score) == 0.0 and states.tolist() == [1, 1]
    # two labels, every path equal: the rule is applied per cell, from the end backwards -- the last blank is held for as long as it was
    # reachable (frames 3, 2), entered from the label (frame 1, the only finite predecessor), which was reached by the skip from 1
    lp = np.zeros((4, 4), dtype=np.float32)
    _, states = viterbi(lp, [1, 2], blank=0)
    assert states.tolist() == [1, 3, 4, 4]


def test_repeated_labels_need_the_blank_between():
    lp = np.log(np.full((3, 2), 0.5, dtype=np.float32))
    score, states = viterbi(lp[:2], [1, 1], blank=0)
    assert states is None and score == NEG
    score, states = viterbi(lp, [1, 1], blank=0)
    assert states.tolist() == [1, 2, 3]
    assert float(score) == float(np.float32(np.float32(lp[0, 0] + lp[0, 0]) + lp[0, 0]))


def test_empty_label_single_frame_and_infeasible_inputs():
    lp = np.log(np.array([[[0.25, 0.75]], [[0.5, 0.5]], [[0.125, 0.875]]], dtype=np.float32))       # (3, 1, 2)
    out = align_ref(lp, np.zeros((1, 0), np.int64), [3], [0], blank=1)                                  # L = 0: all blank
    assert out["ok"].tolist() == [1] and out["paths"].tolist() == [[1, 1, 1]] and out["starts"].shape == (1, 0)
    assert out["scores"][0] == np.float32(np.float32(lp[0, 0, 1] + lp[1, 0, 1]) + lp[2, 0, 1])
    out = align_ref(lp, np.array([[0]]), [1], [1], blank=1)                                             # Tb = 1
    assert out["paths"].tolist() == [[0, -1, -1]] and out["frame_scores"][0, 0] == lp[0, 0, 0] and out["ends"].tolist() == [[1]]
    out = align_ref(lp, np.array([[0, 0]]), [2], [2], blank=1)                                          # needs 3 frames
    assert out["ok"].tolist() == [0] and out["scores"][0] == NEG and (out["paths"] == -1).all() and (out["starts"] == -1).all()
    out = align_ref(lp, np.array([[0, 0]]), [0], [0], blank=1)                                          # Tb = 0, L = 0
    assert out["ok"].tolist() == [1] and out["scores"][0] == 0 and (out["paths"] == -1).all()
    out = align_ref(lp, np.array([[0, 0]]), [0], [1], blank=1)
    assert out["ok"].tolist() == [0] and out["scores"][0] == NEG
    out = align_ref(lp, np.array([[0, 0]]), [4], [1], blank=1)                                          # lengths outside the tensors
    assert out["ok"].tolist() == [0] and np.isnan(out["scores"][0]) and (out["paths"] == -1).all()
    lp2 = lp.copy()
    lp2[1, 0, 0] = NEG                                                                                  # the label cannot sit on frame 1
    out = align_ref(lp2, np.array([[0]]), [3], [1], blank=1)
    assert out["ok"].tolist() == [1] and out["paths"].tolist() in ([[0, 1, 1]], [[1, 1, 0]])
    lp2[:, 0, 0] = NEG
    assert align_ref(lp2, np.array([[0]]), [3], [1], blank=1)["ok"].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------
# argument errors before any device work
# ---------------------------------------------------------------------------------------------------------
def test_forced_align_argument_errors_come_before_the_device():
    from ctc_pytorch_amd import ops
    lp = torch.log_softmax(torch.randn(6, 2, 5), -1)
    tg = torch.tensor([[1, 2], [3, 0]])
    for blank in (-1, 5, 9):
        with pytest.raises(ValueError, match="blank"):
            ops.ctc_forced_align(lp, tg, [6, 5], [2, 1], blank=blank)
    with pytest.raises(ValueError, match="batch size"):
        ops.ctc_forced_align(lp, tg, [6, 5, 4], [2, 1])
    with pytest.raises(ValueError, match="input_lengths"):
        ops.ctc_forced_align(lp, tg, [7, 5], [2, 1])
    with pytest.raises(ValueError, match="target_lengths"):
        ops.ctc_forced_align(lp, tg, [6, 5], [3, 1])
    with pytest.raises(ValueError):
        ops.ctc_forced_align(lp, torch.tensor([1, 2]), [6, 5], [2, 1])             # concatenated: fewer targets than the lengths say
    with pytest.raises(ValueError):
        ops.ctc_forced_align(lp[0, 0], tg, [6, 5], [2, 1])
    # valid arguments on the host: no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_forced_align(lp, tg, [6, 5], [2, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_forced_align(lp[:, 0], torch.tensor([1, 2]), 6, 2, blank=4)


def test_align_entry_point_rejects_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    from ctc_pytorch_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        ge.build()
    L = _lib.lib()
    buf = torch.zeros(1 << 12)
    p = buf.data_ptr()
    T, B, V, Lmax = 4, 2, 5, 2
    assert L.ctcn_ctc_align_ws_bytes(T, B, Lmax) == 0 and L.ctcn_ctc_align_ws_bytes(800, 32, 60) == 0      # rows in LDS: no workspace
    assert L.ctcn_ctc_align_ws_bytes(0, B, Lmax) == 0 and L.ctcn_ctc_align_ws_bytes(T, B, -1) == 0
    assert L.ctcn_ctc_align_ws_bytes(2200, 2, 2047) == 2 * 2200 * 256 * 4                                   # (B, T, ceil(S / 16)) words
    assert L.ctcn_ctc_align_ws_bytes(20000, 3, 1) == 3 * 20000 * 4
    for blank in (-1, V, V + 3):
        assert L.ctcn_ctc_align(p, p, p, p, p, p, p, p, p, p, T, B, V, Lmax, blank, None, 0, None) == -1
        assert b"blank" in L.ctcn_last_error()
    for k in range(8):                                           # every required pointer (starts / ends may be NULL)
        args = [p] * 10
        args[k] = None
        assert L.ctcn_ctc_align(*args, T, B, V, Lmax, 0, None, 0, None) == -1, k
    for dims in ((0, B, V, Lmax), (T, 0, V, Lmax), (T, B, 0, Lmax), (T, B, V, -1)):
        assert L.ctcn_ctc_align(p, p, p, p, p, p, p, p, p, p, *dims, 0, None, 0, None) == -1
    assert L.ctcn_ctc_align(p, p, p, p, p, p, p, p, p, p, T, B, V, 2048, 0, None, 0, None) == -3
    assert b"2047" in L.ctcn_last_error()
    # back-pointer rows that do not fit in LDS want the workspace of the size query
    assert L.ctcn_ctc_align(p, p, p, p, p, p, p, p, p, p, 2200, 2, V, 2047, 0, None, 0, None) == -1
    assert L.ctcn_ctc_align(p, p, p, p, p, p, p, p, p, p, 2200, 2, V, 2047, 0, p, 1024, None) == -4


# ---------------------------------------------------------------------------------------------------------
# host half of Decoder.align
# ---------------------------------------------------------------------------------------------------------
def test_decoder_spans_from_arrays():
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder, Decoder, GreedyDecoder
    assert GreedyDecoder.align is Decoder.align and BeamDecoder.align is Decoder.align
    d = GreedyDecoder({0: "_", 1: "a", 2: "b", 3: "c"}, space_idx=-1, blank_index=0)
    fs = np.array([[-1.0, -2.0, -0.5, -0.25, -4.0, 0.0], [0.0] * 6, [-0.5, -1.5, 0, 0, 0, 0]], dtype=np.float32)
    starts = np.array([[0, 3], [-1, -1], [-1, -1]], dtype=np.int32)
    ends = np.array([[2, 4], [-1, -1], [-1, -1]], dtype=np.int32)
    out = d._spans(fs, np.array([-7.75, -np.inf, -2.0], np.float32), np.array([1, 0, 1], np.int32), starts, ends,
                   [np.array([2, 1]), np.array([3]), np.array([], dtype=np.int64)], frame_stride=4)
    assert out[0] == ([("b", 0, 8, -1.5), ("a", 12, 16, -0.25)], -7.75)
    assert out[1] is None
    assert out[2] == ([], -2.0)
