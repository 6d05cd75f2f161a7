"""Timed, scored recognition output on the HIP kernel (ctcn_path_tokens through ops.path_tokens, GreedyDecoder / BeamDecoder.decode_timed and the
decode driver's `ctm` key) against the numpy restatement of tests/path_tokens_ref.py, ops.greedy_collapse, ops.ctc_forced_align and
Decoder.align.

Bounds: the integers and min_lp are compared exactly (the kernel's max and min are exact); mean_lp, mean_margin and path_score within
1e-6 * max(1, |ref|): the one rounding to float32 is 6e-8 relative, the double accumulation is negligible, the rest is margin."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_tokens_ref as R  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.testing import synth  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
INT_KEYS, EXACT_KEYS, CLOSE_KEYS = ("ids", "lengths", "starts", "ends"), ("min_lp",), ("mean_lp", "mean_margin", "path_score")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def make_lp(seed, T, B, V, minus_inf=True):
    rs = np.random.RandomState(seed)
    z = (3.0 * rs.standard_normal((T, B, V))).astype(np.float64)
    lp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    if minus_inf and V > 2:
        lp[rs.random_sample((T, B, V)) < 0.01] = -np.inf               # a -inf must stay inside its own token
    return lp


def make_paths(seed, T, B, V, blank, lens):
    """(B, T) paths that hold what the kernel can get wrong: runs across every multiple of 64, tokens that start on frame 64 m - 1 and on 64 m, a
    run that ends exactly at n (and goes on behind it), `a _ a`, ids outside [0, V), an all-blank and a single-label utterance."""
    rs = np.random.RandomState(seed)
    labels = [c for c in range(V) if c != blank]
    pick = lambda: labels[rs.randint(len(labels))] if labels else blank
    path = np.full((B, T), blank, dtype=np.int32)
    for b in range(B):
        t = 0
        while t < T:                                                    # random runs of labels and blanks, 1 .. 5 frames each
            run = rs.randint(1, 6)
            path[b, t:t + run] = blank if rs.random_sample() < 0.4 else pick()
            t += run
        path[b, rs.choice(T, T // 10 + 1, replace=False)] = -1         # outside [0, V): blank, never an index
        path[b, rs.choice(T, T // 20 + 1, replace=False)] = V + 3
        a, c = pick(), pick()
        for m in range(64, T + 1, 64):
            if b % 3 == 0 and m + 3 <= T:                               # one run over the boundary
                path[b, m - 5] = blank
                path[b, m - 4:m + 3] = a
            elif b % 3 == 1 and m + 2 <= T:                             # a token that starts on frame 64 m - 1
                path[b, m - 2] = blank
                path[b, m - 1:m + 2] = a
            elif b % 3 == 2 and m + 2 <= T:                             # a token that starts on frame 64 m, behind another label
                path[b, m - 1] = c
                path[b, m:m + 2] = a if a != c or not labels else labels[(labels.index(a) + 1) % len(labels)]
        if T >= 3:
            path[b, :3] = [a, blank, a]
        n = min(max(int(lens[b]), 0), T)
        if n >= 2:
            path[b, n - 2:min(n + 2, T)] = c                            # ends exactly at n; the same label behind n must not be seen
    if B > 2:
        path[2] = blank
    if B > 3:
        path[3] = pick()
    return path


def run_raw(path, lens, lp, blank, dev):
    """ctcn_path_tokens called directly on a time-major contiguous path, every output pre-filled with a sentinel."""
    T, B, V = lp.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    path_d = torch.from_numpy(np.ascontiguousarray(path.T)).to(dev)
    lp_d, lens_d = torch.from_numpy(lp).to(dev), torch.as_tensor(lens, dtype=torch.int32).to(dev)
    ints = {k: torch.full((B, T), -7777, dtype=torch.int32, device=dev) for k in ("ids", "starts", "ends")}
    vals = {k: torch.full((B, T), 12345.0, dtype=torch.float32, device=dev) for k in ("mean_lp", "min_lp", "mean_margin")}
    n, score = torch.full((B,), -7777, dtype=torch.int32, device=dev), torch.full((B,), 12345.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ctcn_path_tokens(p(path_d), B, 1, p(lp_d), p(lens_d), p(ints["ids"]), p(n), p(ints["starts"]), p(ints["ends"]),
                                           p(vals["mean_lp"]), p(vals["min_lp"]), p(vals["mean_margin"]), p(score), T, B, V, blank,
                                           _lib.stream_ptr()), "path_tokens")
    out = dict(ints, lengths=n, path_score=score, **vals)
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(got, ref, tag):
    for k in INT_KEYS + EXACT_KEYS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (tag, k, got[k], ref[k])
    for k in CLOSE_KEYS:
        g, r = got[k].astype(np.float64), ref[k].astype(np.float64)
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin], r[~fin], equal_nan=True), (tag, k, "non-finite entries")
        err = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        worst = float(err.max()) if err.size else 0.0
        print("%s %s: max err / max(1, |ref|) = %.3g" % (tag, k, worst))
        assert worst <= 1e-6, (tag, k, worst)


@pytest.mark.parametrize("V", [1, 2, 62, 65, 130])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 257, 600])
def test_against_the_numpy_restatement(dev, T, V):
    """Three blanks x (time-major, batch-major) x (contiguous, strided view), the six lengths dealt to the six utterances in another rotation
    each time; once through the C entry with every output pre-filled (every element is written)."""
    B, base_lens = 6, [0, 1, 64, 65, T - 1, T]
    lp = make_lp(100 * T + V, T, B, V)
    lp_d = torch.from_numpy(lp).to(dev)
    combos = [(blank, bm) for blank in sorted({0, V // 2, V - 1}) for bm in (False, True)]
    for i, (blank, batch_major) in enumerate(combos):
        lens = base_lens[i:] + base_lens[:i]
        path = make_paths(7 * T + V + i, T, B, V, blank, lens)
        ref = R.path_tokens(path, lens, lp, blank)
        if i == 0:
            got = run_raw(path, lens, lp, blank, dev)
            assert (got["ids"] != -7777).all() and (got["starts"] != -7777).all() and (got["ends"] != -7777).all() and (got["lengths"] != -7777).all()
            assert all((got[k] != 12345.0).all() for k in ("mean_lp", "min_lp", "mean_margin", "path_score"))
            compare(got, ref, "raw T%d V%d" % (T, V))
        if (i // 2 + i) % 2 == 0:                                       # a strided view: every other column of a wider buffer, behind an offset
            wide = torch.full((B, 2 * T + 3) if batch_major else (T, 2 * B + 3), -5, dtype=torch.int32, device=dev)
            view = wide[:, 3::2][:, :T] if batch_major else wide[:, 3::2][:, :B]
            view.copy_(torch.from_numpy(path if batch_major else np.ascontiguousarray(path.T)))
        else:
            view = torch.from_numpy(path if batch_major else np.ascontiguousarray(path.T)).to(dev)
        pt = ops.path_tokens(view, lens if i % 3 else torch.tensor(lens, device=dev), lp_d, blank=blank, batch_major=batch_major)
        got = {k: getattr(pt, k).cpu().numpy() for k in pt._fields}
        compare(got, ref, "T%d V%d blank%d %s" % (T, V, blank, "bt" if batch_major else "tb"))


def test_ids_and_lengths_are_greedy_collapse_s(dev):
    T, B, V = 130, 5, 62
    lp = torch.from_numpy(make_lp(5, T, B, V, minus_inf=False)).to(dev)
    lp[:, :, 0] += 6.0                                                  # blanks and repeats among the arg-max frames
    lp[:, :, 5] += 5.0
    lens = [130, 1, 64, 65, 129]
    idx = ops.argmax_last(lp)
    for blank in (0, 7):
        ids, n = ops.greedy_collapse(idx, lens, blank=blank)
        pt = ops.path_tokens(idx, lens, lp, blank=blank)
        assert torch.equal(pt.lengths, n) and int(n.max()) > 20
        for b in range(B):
            assert torch.equal(pt.ids[b, :int(n[b])], ids[b, :int(n[b])])
    assert int((idx == 0).sum()) > 50 and int(((idx[1:] == idx[:-1]) & (idx[1:] != 0)).sum()) > 10


def test_consistent_with_the_forced_alignment_of_its_own_tokens(dev):
    """Log-probs whose best class leads every frame by >= 0.1 (0.2 in the logits, and log-softmax keeps differences): any other path of the
    same labels loses >= 0.1, far above the float32 error of a 96-term chain, so the alignment of the greedy ids IS the arg-max path."""
    T, B, V = 96, 4, 8
    rs = np.random.RandomState(11)
    lens = [96, 50, 1, 77]
    best = make_paths(3, T, B, V, 0, lens).clip(0, V - 1)
    best[2], best[3] = make_paths(4, T, 2, V, 0, lens[2:]).clip(0, V - 1)   # no all-blank / single-label rows here
    z = -rs.random_sample((T, B, V))
    np.put_along_axis(z, best.T[:, :, None].astype(np.int64), 0.2, axis=2)
    lp = torch.from_numpy((z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)).to(dev)
    idx = ops.argmax_last(lp)
    assert np.array_equal(idx.cpu().numpy(), best.T)
    ids, n = ops.greedy_collapse(idx, lens, blank=0)
    Lmax = int(n.max())
    tg = torch.where(torch.arange(Lmax, device=dev)[None, :] < n[:, None], ids[:, :Lmax], torch.zeros_like(ids[:, :Lmax])).to(torch.int64)
    a = ops.ctc_forced_align(lp, tg, lens, n.to(torch.int64), blank=0)
    assert bool(a.ok.all())
    want = idx.t().clone()
    for b in range(B):
        want[b, lens[b]:] = -1
    assert torch.equal(a.paths, want)
    pt = ops.path_tokens(a.paths, lens, lp, blank=0, batch_major=True)
    assert torch.equal(pt.lengths, n)
    assert torch.equal(pt.starts[:, :Lmax], a.starts) and torch.equal(pt.ends[:, :Lmax], a.ends)
    live = pt.starts >= 0
    assert int(live.sum()) == int(n.sum()) and float(pt.mean_margin[live].min()) >= 0.1
    sc = torch.stack([a.frame_scores[b, :lens[b]].double().sum() for b in range(B)]).cpu().numpy()
    assert np.allclose(pt.path_score.cpu().numpy(), sc, rtol=1e-6, atol=0)


@pytest.fixture(scope="module")
def decoders():
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder, GreedyDecoder
    i2c = synth.int2char(62)
    return (GreedyDecoder(i2c, space_idx=-1, blank_index=0),
            BeamDecoder(i2c, beam_width=20, blank_index=0, space_idx=-1, lm_path=os.path.join(G, "lm_phone_bg.arpa")))


def test_decoders_time_what_they_decode(dev, decoders):
    T, B, V = 60, 6, 62
    lp = torch.from_numpy(synth.make_logprobs(21, T, B, V, "peaky")).to(dev)
    lens = [60, 37, 30, 59, 44, 25]
    greedy, beam = decoders
    for dec, join in ((greedy, lambda ph: "".join(" " + p for p in ph)), (beam, lambda ph: " ".join(ph))):
        strings = dec.decode(lp, lens)
        timed = dec.decode_timed(lp, lens)
        assert len(timed) == B and all(e is not None for e in timed)
        assert [join([tok[0] for tok in e[0]]) for e in timed] == strings
        assert sum(len(e[0]) for e in timed) > B
        for b, (toks, score) in enumerate(timed):
            edges = [0] + [v for _, s, e, _ in toks for v in (s, e)] + [lens[b]]
            assert all(x <= y for x, y in zip(edges, edges[1:])) and all(s < e for _, s, e, _ in toks)      # ordered, disjoint, inside the utterance
            assert all(0.0 < c <= 1.0 for _, _, _, c in toks) and score <= 0.0
        by3 = dec.decode_timed(lp, lens, frame_stride=3)
        assert [[(p, 3 * s, 3 * e, c) for p, s, e, c in e[0]] for e in timed] == [e[0] for e in by3] and [e[1] for e in timed] == [e[1] for e in by3]
        full = dec.decode_timed(lp, lens, detail=True)
        assert [[tok[:4] for tok in e[0]] for e in full] == [e[0] for e in timed]
        assert all(len(tok) == 6 and tok[4] <= np.log(tok[3]) + 1e-6 for e in full for tok in e[0])          # min_lp <= mean_lp
    # the beam's spans are those of Decoder.align on its own hypothesis; the greedy ones are the arg-max runs, where the lead is >= 0
    hyp, _ = beam._decoder.decode_ids(lp, lens)
    ali = beam.align(lp, lens, np.concatenate([np.asarray(h, dtype=np.int64) for h in hyp]), [len(h) for h in hyp])
    timed = beam.decode_timed(lp, lens)
    for (toks, score), (spans, ali_score) in zip(timed, ali):
        assert [t[:3] for t in toks] == [s[:3] for s in spans]
        assert np.allclose([np.log(t[3]) for t in toks], [s[3] for s in spans], rtol=1e-5, atol=1e-6) and abs(score - ali_score) <= 1e-5 * max(1.0, abs(ali_score))
    assert all(tok[5] >= 0.0 for e in greedy.decode_timed(lp, lens, detail=True) for tok in e[0])
    # an utterance whose search ends with a status (one frame, no label: the reference's IndexError in decode) has no entry; the others do
    short = beam.decode_timed(lp, [60, 37, 1] + lens[3:])
    assert short[2] is None and short[:2] + short[3:] == timed[:2] + timed[3:]
    assert greedy.decode_timed(lp, [60, 37, 0] + lens[3:])[2] == ([], 0.0)


def test_beam_decode_timed_defaults_to_full_length(dev, decoders):
    T, B, V = 20, 2, 62
    lp = torch.from_numpy(synth.make_logprobs(22, T, B, V, "peaky")).to(dev)
    assert decoders[1].decode_timed(lp) == decoders[1].decode_timed(lp, [T, T])


@pytest.mark.parametrize("kind", ["greedy", "beam"])
def test_decode_driver_writes_the_tokens_of_decode_timed_and_scores_as_without(dev, kind, tmp_path):
    """steps/decode_ctc.decode_and_score with `ctm` on, over one ragged minibatch of a tiny model with a stride-2 front-end, as
    tests/test_length_mask.py drives it."""
    from test_length_mask import batch, build
    LENS = [40, 21, 17, 40, 9, 26]                                      # T = 40, ragged; every utterance long enough for the search to say a phone
    from ctc_pytorch_amd.steps import decode_ctc
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder, GreedyDecoder
    from ctc_pytorch_amd.utils.ctm import read_ctm, write_ctm
    V, T = 9, max(LENS)
    m, _ = build("LSTM", True, dev)
    out_lens = m.output_lengths(LENS)
    x, tg, tl = batch(LENS, T, 12, V, out_lens)
    frac = torch.tensor([np.float32(float(l) / float(T)) for l in LENS])
    words = synth.int2char(V)
    utts = ["spk%d_utt%d" % (b % 2, 9 - b) for b in range(len(LENS))]
    data = [(x, frac, tg, tl, utts)]

    def make():
        if kind == "greedy":
            return GreedyDecoder(words, space_idx=-1, blank_index=0)
        arpa = str(tmp_path / "lm.arpa")
        synth.write_arpa(arpa, [words[i] for i in range(1, V)], seed=3, n_bigrams=30)
        return BeamDecoder(words, beam_width=5, blank_index=0, space_idx=-1, lm_path=arpa)

    off_log, on_log = [], []
    off = decode_ctc.decode_and_score(m, data, make(), words, dev, log=off_log.append, mask_padding=True)
    path = str(tmp_path / "hyp.ctm")
    on = decode_ctc.decode_and_score(m, data, make(), words, dev, log=on_log.append, mask_padding=True, ctm=path, ctm_frame_shift=0.01,
                                     n_skip_frame=2)
    assert on == off and on_log == off_log
    assert decode_ctc.input_frames_per_output_frame(m) == 2
    with torch.no_grad():
        probs = m.eval()(x.to(dev), input_lengths=torch.tensor(LENS))
    timed = make().decode_timed(probs, out_lens.tolist(), frame_stride=4)     # front-end stride 2 x frame skip 2
    want = io.StringIO()
    assert write_ctm(want, utts, timed, frame_shift=0.01) >= len(LENS)              # (the seeded model says at least one phone per utterance)
    assert open(path).read() == want.getvalue()
    back = read_ctm(open(path))
    assert [u for u in utts if u in back] == list(back)
    for u, e in zip(utts, timed):
        assert [t[0] for t in back.get(u, [])] == [t[0] for t in e[0]]
        assert all(abs(t[1] - 0.01 * s[1]) <= 5.01e-4 and s[1] % 4 == 0 and s[2] % 4 == 0 for t, s in zip(back.get(u, []), e[0]))
