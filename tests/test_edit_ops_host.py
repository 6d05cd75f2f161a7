"""Host-side checks of the error breakdown (no GPU): the restatement of the definition itself (tests/edit_ops_ref.py), the library's host
alignment ctcn_levenshtein_ops against it, the phone fold table, ErrorStats, and the drivers' `error_report` / `score_map` keys."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ops_ref as R  # noqa: E402
from ctc_pytorch_amd import _lib  # noqa: E402
from ctc_pytorch_amd.utils import scoring  # noqa: E402

MAP_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phones.60-48-39.map")


def _ragged(seed, n, max_len, alphabet):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, alphabet, rng.randint(0, max_len + 1)).tolist(), rng.randint(0, alphabet, rng.randint(0, max_len + 1)).tolist())
            for _ in range(n)]


def _host_ops(hyp, ref, want_ali=True):
    """ctcn_levenshtein_ops called directly: (return value, counts4, ali (nh + nr, 2))."""
    h, r = np.asarray(hyp, dtype=np.int32), np.asarray(ref, dtype=np.int32)
    counts = np.full(4, -7, dtype=np.int64)
    ali = np.full((len(h) + len(r) + 1, 2), -9, dtype=np.int32)            # one guard row behind the (nh + nr, 2) the entry may write
    n = _lib.lib().ctcn_levenshtein_ops(h.ctypes.data, len(h), r.ctypes.data, len(r), counts.ctypes.data, ali.ctypes.data if want_ali else None)
    assert (ali[-1] == -9).all()
    return n, counts.tolist(), ali[:-1]


def test_restatement_is_a_valid_edit_script_with_the_three_invariants():
    """The pairs rebuild both (mapped) sequences in order; sub + del + cor == ref_len', sub + ins + cor == hyp_len', sub + del + ins == the
    distance -- on every pair over {0, 1, 2} of length <= 4 and on random ragged pairs under a map that folds, drops and passes through."""
    hyps, refs, counts, ali, ali_len, conf = R.exhaustive()
    assert len(hyps) == 121 * 121
    cmap = [0, 1, 1, -1, 4]                                               # 2 folds into 1, 3 is dropped, ids >= 5 pass through
    cases = [(h, r, None) for h, r in zip(hyps, refs)] + [(h, r, cmap) for h, r in _ragged(3, 200, 12, 7)]
    for h, r, m in cases:
        c, ops, dist = R.edit_ops(h, r, m)
        hm, rm = R.apply_map(h, m), R.apply_map(r, m)
        assert [x for mv, _, x in ops if mv != 1] == hm and [a for mv, a, _ in ops if mv != 2] == rm
        assert all((mv == 1) == (x == -1 and mv != 0) and (mv == 2) == (a == -1 and mv != 0) for mv, a, x in ops)
        sub, dele, ins, cor, nh, nr = c
        assert (nh, nr) == (len(hm), len(rm))
        assert sub + dele + cor == nr and sub + ins + cor == nh and sub + dele + ins == dist
    assert 3 not in sum((R.apply_map(h, cmap) for h, _ in _ragged(3, 200, 12, 7)), []) and conf[3, 3] == 0
    assert conf.sum() == ali_len.sum() and (counts[:, :4].sum(1) == ali_len).all()


def test_restatement_pinned_ties():
    assert R.edit_ops([1], [1, 1])[1] == [(1, 1, -1), (0, 1, 1)]                      # del r0, cor
    assert R.edit_ops([7, 8], [8, 7])[1] == [(0, 8, 7), (0, 7, 8)]                    # sub, sub
    assert R.edit_ops([], [4, 5])[1] == [(1, 4, -1), (1, 5, -1)] and R.edit_ops([4, 5], [])[1] == [(2, -1, 4), (2, -1, 5)]


def test_row_at_a_time_table_equals_the_literal_one():
    seqs = R.small_sequences()
    for h in seqs[::3]:
        for r in seqs[::2]:
            assert np.array_equal(R.table_rows(h, r), R.table_literal(h, r))
    for h, r in _ragged(11, 60, 40, 4):
        assert np.array_equal(R.table_rows(h, r), R.table_literal(h, r))


def test_host_alignment_equals_the_restatement():
    """ctcn_levenshtein_ops: counts, pairs, the -1 fill and the return value equal the restatement, and its distance is ctcn_levenshtein's."""
    L = _lib.lib()
    hyps, refs, counts, ali, ali_len, _ = R.exhaustive()
    for b in range(len(hyps)):
        n, c, a = _host_ops(hyps[b], refs[b])
        assert n == ali_len[b] and c == counts[b, :4].tolist()
        assert np.array_equal(a, ali[b, :len(hyps[b]) + len(refs[b])]), (hyps[b], refs[b])
    for h, r in _ragged(5, 300, 60, 5) + _ragged(6, 20, 300, 3):
        want_c, ops, dist = R.edit_ops(h, r, table=R.table_rows)
        n, c, a = _host_ops(h, r)
        assert n == len(ops) and c == want_c[:4]
        assert a[:n].tolist() == [[x, y] for _, x, y in ops] and (a[n:] == -1).all()
        ha, ra = np.asarray(h, dtype=np.int32), np.asarray(r, dtype=np.int32)
        assert c[0] + c[1] + c[2] == dist == L.ctcn_levenshtein(ha.ctypes.data, len(h), ra.ctypes.data, len(r))
        assert _host_ops(h, r, want_ali=False)[:2] == (n, c)
    # the Python face: the map is applied first
    c4, pairs = scoring.align_ids([0, 2, 3, 9], [1, 3, 3, 9, 2], class_map=[0, 1, 1, -1])
    want_c, ops, _ = R.edit_ops([0, 2, 3, 9], [1, 3, 3, 9, 2], [0, 1, 1, -1])
    assert list(c4) == want_c[:4] and pairs.tolist() == [[a, b] for _, a, b in ops]
    assert scoring.align_ids([], [])[0] == (0, 0, 0, 0) and scoring.align_ids([], [], alignment=False)[1] is None


def test_host_alignment_argument_errors():
    L = _lib.lib()
    x = np.zeros(4, dtype=np.int32)
    c = np.zeros(4, dtype=np.int64)
    assert L.ctcn_levenshtein_ops(x.ctypes.data, 2, x.ctypes.data, 2, None, None) == -1            # a NULL counts4 is a bad argument
    assert L.ctcn_levenshtein_ops(None, 2, x.ctypes.data, 2, c.ctypes.data, None) == -1
    assert L.ctcn_levenshtein_ops(x.ctypes.data, 2, None, 2, c.ctypes.data, None) == -1
    assert L.ctcn_levenshtein_ops(x.ctypes.data, -1, x.ctypes.data, 2, c.ctypes.data, None) == -1
    assert L.ctcn_levenshtein_ops(x.ctypes.data, 2, x.ctypes.data, -1, c.ctypes.data, None) == -1
    assert L.ctcn_levenshtein_ops(None, 0, None, 0, c.ctypes.data, None) == 0 and c.tolist() == [0, 0, 0, 0]
    # the device entry and its workspace query before they touch a device
    assert L.ctcn_edit_ops_ws_bytes(0, 0, 0) == 0 and L.ctcn_edit_ops_ws_bytes(4, 40, 7) == 0 and L.ctcn_edit_ops_ws_bytes(3, 1200, 300) > 0
    assert L.ctcn_edit_ops(*([None] * 5), 0, *([None] * 4), 0, 0, 0, 0, None, 0, None) == -1
    from ctc_pytorch_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edit_ops(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2))


def test_load_phone_map_on_the_reference_table():
    rows = [line.split() for line in open(MAP_FILE)]
    assert len(rows) == 61
    names = ["blank"] + sorted({n for row in rows for n in row})           # one vocabulary that holds the 60, 48 and 39 sets
    ids = {n: k for k, n in enumerate(names)}
    m39 = scoring.load_phone_map(MAP_FILE, "60-39", names)
    assert m39.dtype == np.int32 and m39.shape == (len(names),)
    assert m39[ids["q"]] == -1 and m39[ids["ao"]] == ids["aa"] and m39[ids["zh"]] == ids["sh"] and m39[ids["blank"]] == ids["blank"]
    for closure in ("bcl", "dcl", "gcl", "kcl", "pcl", "tcl", "epi", "pau", "h#"):         # (vcl / cl are names of the 48 set: below)
        assert m39[ids[closure]] == ids["sil"], closure
    m48 = scoring.load_phone_map(MAP_FILE, "60-48", names)
    assert m48[ids["q"]] == -1 and m48[ids["ao"]] == ids["ao"] and m48[ids["bcl"]] == ids["vcl"] and m48[ids["kcl"]] == ids["cl"]
    m4839 = scoring.load_phone_map(MAP_FILE, "48-39", names)
    assert m4839[ids["q"]] == ids["q"]                                     # not a name of the 48 set: absent from the source column
    assert m4839[ids["vcl"]] == m4839[ids["cl"]] == ids["sil"] and m4839[ids["ao"]] == ids["aa"] and m4839[ids["zh"]] == ids["sh"]
    assert len({int(m39[ids[r[0]]]) for r in rows} - {-1}) == 39 and len({int(m48[ids[r[0]]]) for r in rows} - {-1}) == 48
    for row in rows:                                                       # the file's own statement, line by line
        assert m39[ids[row[0]]] == (ids[row[2]] if len(row) == 3 else -1)
    as_dict = scoring.load_phone_map(MAP_FILE, "60-39", {k: n for k, n in enumerate(names)})
    assert np.array_equal(as_dict, m39)
    with pytest.raises(ValueError, match="sil"):
        scoring.load_phone_map(MAP_FILE, "60-39", [n for n in names if n != "sil"])
    with pytest.raises(ValueError, match="cols"):
        scoring.load_phone_map(MAP_FILE, "39-48", names)


def test_error_stats_merge_state_round_trip_and_report():
    words = ["blank", "aa", "b", "k", "sil"]
    V = len(words)
    tab = np.zeros((V + 1, V + 1), dtype=np.int64)
    tab[1, 1], tab[2, 2], tab[3, 3] = 50, 30, 17                          # correct pairs
    tab[1, 2], tab[2, 1], tab[3, 2] = 4, 6, 1                             # aa -> b 4, b -> aa 6, k -> b 1
    tab[4, V], tab[1, V] = 3, 2                                           # deletions: sil 3, aa 2
    tab[V, 3] = 5                                                         # insertions: k 5
    a = scoring.ErrorStats(words)
    a.add(np.array([[6, 2, 1, 40, 47, 48], [5, 3, 4, 57, 66, 65]]), tab)
    assert a.totals() == {"sub": 11, "del": 5, "ins": 5, "cor": 97, "hyp_len": 113, "ref_len": 113, "errors": 21, "per": 100.0 * 21 / 113}
    assert a.report(top=2).splitlines() == [
        "%PER 18.58 [ 21 / 113, 5 ins, 5 del, 11 sub ]",
        "confusions (reference -> hypothesis): b -> aa 6, aa -> b 4",
        "deletions: sil 3, aa 2",
        "insertions: k 5"]
    assert "k -> b 1" in a.report() and scoring.ErrorStats(words).report().splitlines()[1:] == [
        "confusions (reference -> hypothesis): none", "deletions: none", "insertions: none"]
    st = a.state()
    assert st.dtype == torch.int64 and st.shape == (6 + (V + 1) ** 2,) and st[:6].tolist() == [11, 5, 5, 97, 113, 113]
    b = scoring.ErrorStats.from_state(words, st)
    assert torch.equal(b.state(), st) and np.array_equal(b.confusion.numpy(), tab)
    b.merge(a)
    assert torch.equal(b.state(), 2 * st)                                 # what one all-reduce over two equal ranks gives
    st[0] = 99
    assert a.totals()["sub"] == 11                                        # state() is a copy
    c4 = scoring.ErrorStats(words).add([1, 2, 3, 4])                      # the host alignment's four counts: lengths by the invariants
    assert c4.state()[:6].tolist() == [1, 2, 3, 4, 8, 7]
    with pytest.raises(ValueError):
        a.merge(scoring.ErrorStats(words[:-1]))
    with pytest.raises(ValueError):
        scoring.ErrorStats.from_state(words, st[:-1])
    # pairs of a host alignment: members outside [0, V) are counted but not entered
    p = scoring.ErrorStats(words)
    counts, pairs = scoring.align_ids([1, 2, 9, 3], [1, 3, 9, 3, 4])
    p.add_pairs(counts, pairs)
    want_c, ops, _ = R.edit_ops([1, 2, 9, 3], [1, 3, 9, 3, 4])
    assert p.state()[:6].tolist() == want_c and np.array_equal(p.confusion.numpy(), R.confusion([ops], V))
    assert p.confusion.sum() == len(ops) - 1


class _StubModel(torch.nn.Module):
    def __init__(self, T, B, V):
        super().__init__()
        self.shape = (T, B, V)

    def forward(self, *args, **kwargs):
        return torch.zeros(*self.shape)

    def output_lengths(self, frames):
        return torch.as_tensor(frames)


def test_decode_driver_scores_through_a_proxy_and_logs_the_report_after_the_totals():
    from ctc_pytorch_amd.steps import decode_ctc
    from ctc_pytorch_amd.utils.ctcDecoder import Decoder
    words = {0: "blank", 1: "aa", 2: "ao", 3: "b", 4: "q"}
    cmap = np.array([0, 1, 1, 3, -1], dtype=np.int32)                      # ao folds into aa, q is dropped
    T, B, V = 8, 2, 5

    class Dec(Decoder):
        def decode(self, probs, lens):
            return [" aa b q", " ao zz"]                                   # "zz": a word outside the vocabulary

    data = [(torch.zeros(B, T, V), torch.ones(B), torch.tensor([[2, 3, 0], [1, 3, 3]]), torch.tensor([2, 3]), ["u0", "u1"])]
    plain_log, log = [], []
    plain = Dec(words, space_idx=-1)
    want = decode_ctc.decode_and_score(_StubModel(T, B, V), data, plain, words, "cpu", log=plain_log.append, mask_padding=False)
    dec, stats = Dec(words, space_idx=-1), scoring.ErrorStats(words)
    got = decode_ctc.decode_and_score(_StubModel(T, B, V), data, dec, words, "cpu", log=log.append, mask_padding=False, stats=stats, class_map=cmap)
    assert got == want and log[:2] == plain_log and len(plain_log) == 2    # the CER / WER lines and the return value are unchanged
    assert (dec.num_word, dec.num_char) == (plain.num_word, plain.num_char) and dec.num_word == 5      # counters written through the proxy
    assert log[2:] == [stats.report()]
    # utterance 0: hyp aa b (q dropped) vs ref ao b -> aa b: two correct; utterance 1: hyp aa zz vs ref aa b b: cor, sub (outside), del b
    u0, u1 = R.edit_ops([1, 3, 4], [2, 3], cmap), R.edit_ops([2, 5], [1, 3, 3], cmap)
    assert stats.state()[:6].tolist() == [a + b for a, b in zip(u0[0], u1[0])] == [1, 1, 0, 3, 4, 5]
    assert np.array_equal(stats.confusion.numpy(), R.confusion([u0[1], u1[1]], V))
    assert log[2].splitlines()[0] == "%PER 40.00 [ 2 / 5, 0 ins, 1 del, 1 sub ]"
    proxy = decode_ctc._ScoringDecoder(dec, scoring.ErrorStats(words), words)
    assert proxy.wer(" aa b", " b aa") == dec.wer(" aa b", " b aa") == 2 and proxy.cer("ab", "b") == 1


def _host_epoch(monkeypatch, B, T):
    """run_epoch on the host path, as tests/test_length_mask_host.py drives it: the device ops replaced by torch / host stand-ins."""
    from ctc_pytorch_amd import ops
    calls = []
    monkeypatch.setattr(ops, "argmax_last", lambda out: out.argmax(-1).to(torch.int32))
    monkeypatch.setattr(ops, "greedy_collapse", lambda idx, lens, blank=0: (idx.t().contiguous(), torch.full((B,), T, dtype=torch.int32)))

    def distance(ids, ids_len, tg, tl):
        calls.append("edit_distance")
        return torch.tensor([R.edit_ops(ids[b, :ids_len[b]].tolist(), tg[b, :tl[b]].tolist())[2] for b in range(B)], dtype=torch.int32)

    def breakdown(ids, ids_len, tg, tl, class_map=None, num_classes=None, confusion=None, alignment=False):
        calls.append("edit_ops")
        cm = None if class_map is None else class_map.tolist()
        res = [R.edit_ops(ids[b, :ids_len[b]].tolist(), tg[b, :tl[b]].tolist(), cm) for b in range(B)]
        confusion += torch.from_numpy(R.confusion([r[1] for r in res], num_classes))
        return ops.EditOps(torch.tensor([r[0] for r in res], dtype=torch.int32), None, None)

    monkeypatch.setattr(ops, "edit_distance", distance)
    monkeypatch.setattr(ops, "edit_ops", breakdown)
    return calls


class _EpochModel(torch.nn.Module):
    def __init__(self, V):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(V))

    def forward(self, x):
        return torch.log_softmax(x.transpose(0, 1) + self.w, -1)


def test_error_report_keys_parse_default_off_and_leave_the_log_lines_alone(monkeypatch):
    import yaml
    from ctc_pytorch_amd.steps import train_ctc as TR
    names = ["blank"] + sorted({n for line in open(MAP_FILE) for n in line.split()})
    assert TR.report_options(TR.Config()) == {}
    for text, keys in (("error_report: false\nscore_map: x", []), ("drop_out: 0.1", []), ("error_report: true", ["error_report", "index2word"])):
        o = TR.Config()
        for k, v in yaml.safe_load(text).items():
            setattr(o, k, v)
        assert sorted(TR.report_options(o, names)) == keys
    o = TR.Config()
    o.error_report, o.score_map, o.score_map_cols = True, MAP_FILE, "60-39"
    assert np.array_equal(TR.report_options(o, names)["score_map"], scoring.load_phone_map(MAP_FILE, "60-39", names))
    with pytest.raises(ValueError, match="vocabulary"):
        TR.report_options(o, None)

    T, B, V = 6, 2, 5
    calls = _host_epoch(monkeypatch, B, T)
    torch.manual_seed(0)
    data = [(torch.randn(B, T, V), torch.ones(B), torch.tensor([[1, 2, 3], [4, 4, 0]]), torch.tensor([3, 2]), ["a", "b"]) for _ in range(3)]
    loss_fn = torch.nn.CTCLoss(reduction="sum")

    def run(is_training, **kw):
        log = []
        model = _EpochModel(V)
        opt = torch.optim.SGD(model.parameters(), lr=0.0) if is_training else None
        del calls[:]
        out = TR.run_epoch(4, model, data, loss_fn, "cpu", optimizer=opt, print_every=2, is_training=is_training, log=log.append, **kw)
        return out, log, list(calls)

    # keys off: the lines of today, and only the distance is computed
    (acc, loss), log, seen = run(False)
    errs = sum(R.edit_ops(d[0].argmax(-1)[b].tolist(), d[2][b, :d[3][b]].tolist())[2] for d in data for b in range(B))
    assert log == ["Epoch 4 Valid done, total_loss: %.4f, total_wer: %.4f" % (loss, errs / 15.0)] and seen == ["edit_distance"] * 3
    assert acc == 1 - errs / 15.0
    # training passes: the same launches and lines whether the keys are on or off
    (t_out, t_log, t_seen), (r_out, r_log, r_seen) = run(True), run(True, error_report=True, score_map=[0, 1, 1, 3, -1])
    assert t_out == r_out and t_log == r_log and t_seen == r_seen == ["edit_distance"] * 3
    assert len(t_log) == 2 and t_log[0].startswith("Epoch = 4, step = 2, cur_loss = ") and t_log[1].startswith("Epoch 4 Train done, total_loss: ")
    # validation with the report: same return value, same first line, one extra line; without a map the distance is not computed twice
    (r_acc, r_loss), r_log, r_seen = run(False, error_report=True, index2word=["blank", "aa", "ao", "b", "q"])
    assert (r_acc, r_loss) == (acc, loss) and r_log[0] == log[0] and len(r_log) == 2 and r_seen == ["edit_ops"] * 3
    res = [R.edit_ops(d[0].argmax(-1)[b].tolist(), d[2][b, :d[3][b]].tolist()) for d in data for b in range(B)]
    tot = np.sum([r[0] for r in res], axis=0)
    assert r_log[1].startswith("Epoch 4 Valid error breakdown: " + scoring.ErrorStats.summary_line(tot[0], tot[1], tot[2], tot[5]) + "; confusions")
    assert "\n" not in r_log[1] and tot[0] + tot[1] + tot[2] == errs
    # with a map the breakdown is of the mapped classes; total_wer and the return value stay those of the unmapped ones
    (m_acc, m_loss), m_log, m_seen = run(False, error_report=True, score_map=[0, 1, 1, 3, -1], index2word=["blank", "aa", "ao", "b", "q"])
    assert (m_acc, m_loss) == (acc, loss) and m_log[0] == log[0] and m_seen == ["edit_ops", "edit_distance"] * 3
    mres = [R.edit_ops(d[0].argmax(-1)[b].tolist(), d[2][b, :d[3][b]].tolist(), [0, 1, 1, 3, -1]) for d in data for b in range(B)]
    mt = np.sum([r[0] for r in mres], axis=0)
    assert m_log[1].startswith("Epoch 4 Valid error breakdown (mapped classes): " + scoring.ErrorStats.summary_line(mt[0], mt[1], mt[2], mt[5]) + "; ")
    assert mt[5] < tot[5]                                                  # q left the references
