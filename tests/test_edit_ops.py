"""The error breakdown on the HIP kernel (ctcn_edit_ops through ops.edit_ops, Decoder.error_ops, CTC_Model.compute_error_ops and run_epoch)
against the restatement of tests/edit_ops_ref.py.  Everything is an integer with a fixed tie rule: counts, pairs, pair counts and the
confusion table are compared with ==.  Both homes of the move bits are exercised: LDS (every ordinary shape) and the workspace."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ops_ref as R  # noqa: E402
from ctc_pytorch_amd.testing import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _operands(dev, hyps, refs, lda, ldb, a_len=None, b_len=None, fill=1):
    """Padded operands; what lies past a sequence is `fill` (a symbol of the alphabets used here: reading past a length would show)."""
    a = np.full((len(hyps), lda), fill, dtype=np.int32)
    b = np.full((len(refs), ldb), fill, dtype=np.int64)
    for u, (h, r) in enumerate(zip(hyps, refs)):
        a[u, :len(h)] = h
        b[u, :len(r)] = r
    la = np.asarray([len(h) for h in hyps] if a_len is None else a_len, dtype=np.int32)
    lb = np.asarray([len(r) for r in refs] if b_len is None else b_len, dtype=np.int64)
    return tuple(torch.from_numpy(x).to(dev) for x in (a, la, b, lb))


def _check(dev, hyps, refs, lda, ldb, class_map=None, V=None, a_len=None, b_len=None, table=R.table_rows, want=None):
    """One ops.edit_ops call with pairs and table against the restatement; returns the call's (counts, table) on the host."""
    from ctc_pytorch_amd import ops
    args = _operands(dev, hyps, refs, lda, ldb, a_len, b_len)
    conf = torch.zeros((V + 1, V + 1), dtype=torch.int64, device=dev) if V is not None else None
    got = ops.edit_ops(*args, class_map=None if class_map is None else torch.tensor(class_map, dtype=torch.int32), num_classes=V, confusion=conf,
                       alignment=True)
    counts, ali, ali_len, tab = want if want is not None else R.batch(hyps, refs, lda, ldb, class_map, V, table)
    g_counts, g_ali, g_len = got.counts.cpu().numpy(), got.ali.cpu().numpy(), got.ali_len.cpu().numpy()
    assert g_counts.dtype == np.int32 and g_counts.shape == (len(hyps), 6) and g_ali.shape == (len(hyps), lda + ldb, 2)
    bad = np.nonzero((g_counts != counts).any(1) | (g_len != ali_len) | (g_ali != ali).any((1, 2)))[0]
    assert bad.size == 0, (bad[:5], [(hyps[u], refs[u], g_counts[u].tolist(), counts[u].tolist()) for u in bad[:3]])
    if V is not None:
        assert np.array_equal(conf.cpu().numpy(), tab) and tab[V, V] == 0
    return g_counts, (conf.cpu().numpy() if conf is not None else None)


def _seqs(rs, lens, alphabet):
    return [rs.randint(0, alphabet, n).tolist() for n in lens]


def test_every_pair_of_short_sequences_in_one_call(dev):
    """B = 14 641: every (hypothesis, reference) over {0, 1, 2} of length <= 4; the small alphabet forces ties at every kind of cell."""
    hyps, refs, counts, ali, ali_len, tab = R.exhaustive()
    _check(dev, hyps, refs, 4, 4, V=3, want=(counts, ali, ali_len, tab))


@pytest.mark.parametrize("nr", [0, 1, 63, 64, 65, 128, 129, 256, 257, 512])
def test_reference_lengths_at_the_column_edges(dev, nr):
    """ldb = nr picks the kernel's columns per lane (1, 2, 4, 8); hypotheses of length 0, 1, shorter than, as long as and longer than the
    reference, references at and below ldb; four symbols, so ties abound."""
    rs = np.random.RandomState(nr)
    ref_lens = [nr, nr, nr, nr, nr, max(nr - 1, 0), nr // 2, 0]
    hyp_lens = [0, 1, max(nr - 7, 0), nr, nr + 37, nr + 1, nr // 2 + 3, 5]
    refs = _seqs(rs, ref_lens, 4)
    hyps = _seqs(rs, hyp_lens, 4)
    hyps[3] = [x if rs.rand() < 0.8 else (x + 1) % 4 for x in refs[3]]     # mostly right: long diagonal runs
    _check(dev, hyps, refs, nr + 40, nr, V=4)


def test_lengths_are_clamped_and_a_batch_of_one(dev):
    rs = np.random.RandomState(1)
    hyps, refs = _seqs(rs, [6, 6, 6, 6], 3), _seqs(rs, [5, 5, 5, 5], 3)
    a_len, b_len = [9, -3, 6, 2 ** 31 - 1], [5, 77, -2, -2 ** 40]
    want = R.batch([hyps[0], [], hyps[2], hyps[3]], [refs[0], refs[1], [], []], 6, 5, V=3)
    _check(dev, hyps, refs, 6, 5, V=3, a_len=a_len, b_len=b_len, want=want)
    _check(dev, [[1, 2, 2, 0]], [[2, 2, 1]], 4, 3, V=3)
    _check(dev, [[]], [[]], 3, 2, V=3)


def test_class_maps(dev):
    rs = np.random.RandomState(2)
    hyps, refs = _seqs(rs, [9, 0, 14, 70, 3, 1], 5), _seqs(rs, [7, 5, 14, 66, 0, 1], 5)
    first = [[5] + h for h in hyps]                                        # symbol 5 only ever in front / at the end
    last_r = [r + [5] for r in refs]
    for cmap in ([-1] * 6,                                                 # everything is dropped
                 [0, 1, 2, 3, 4, -1],                                      # drops only the first symbol (of the hypotheses below)
                 [0, 1, 1, 3, 3, 5],                                       # folds 2 into 1 and 4 into 3
                 [3, -1, 0, 0, 2, 1]):                                     # permutes, folds and drops
        c, tab = _check(dev, first, last_r, 72, 68, class_map=cmap, V=6)
        if cmap[0] == -1:
            assert not c.any() and not tab.any()
        if cmap == [0, 1, 2, 3, 4, -1]:
            want = R.batch(hyps, refs, 72, 68, None, 6, R.table_rows)     # the same as never having had the 5s
            assert np.array_equal(c, want[0]) and np.array_equal(tab, want[3])
        if cmap == [0, 1, 1, 3, 3, 5]:
            assert not tab[2].any() and not tab[:, 2].any() and not tab[4].any() and not tab[:, 4].any()


def test_ids_outside_the_classes_pass_through_and_index_nothing(dev):
    """Negative ids and ids >= V: compared as they are, counted, mapped by nothing, entered nowhere -- with and without a map."""
    hyps = [[0, -5, 2, 9, 1], [7, 7, 7], [-1, 0], [2, 1000000]]
    refs = [[0, 2, 9, 1, 3], [7, 1, 7], [0, -1, 3], [1000000, 2]]
    for cmap in (None, [1, 1, -1, 3]):
        c, tab = _check(dev, hyps, refs, 5, 5, class_map=cmap, V=4)
        assert tab.sum() < c[:, :4].sum()


def test_counts_do_not_depend_on_the_optional_outputs_and_tables_accumulate(dev):
    from ctc_pytorch_amd import ops
    rs = np.random.RandomState(3)
    h1, r1, h2, r2 = _seqs(rs, [30] * 5, 6), _seqs(rs, [25] * 5, 6), _seqs(rs, [11] * 7, 6), _seqs(rs, [19] * 7, 6)
    a1, a2 = _operands(dev, h1, r1, 30, 25), _operands(dev, h2, r2, 11, 19)
    full = ops.edit_ops(*a1, num_classes=6, confusion=torch.zeros((7, 7), dtype=torch.int64, device=dev), alignment=True)
    bare = ops.edit_ops(*a1)
    assert bare.ali is None and bare.ali_len is None and torch.equal(bare.counts, full.counts)
    assert torch.equal(ops.edit_ops(*a1, alignment=True).counts, full.counts)
    one, two, both = (torch.zeros((7, 7), dtype=torch.int64, device=dev) for _ in range(3))
    ops.edit_ops(*a1, confusion=one)
    ops.edit_ops(*a2, confusion=two)
    ops.edit_ops(*a1, confusion=both)
    ops.edit_ops(*a2, confusion=both)
    assert torch.equal(both, one + two) and int(one.sum()) == int(full.ali_len.sum())
    with pytest.raises(ValueError):
        ops.edit_ops(*a1, confusion=torch.zeros((7, 7), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.edit_ops(*a1, class_map=[0, 1, 2], num_classes=6)
    with pytest.raises(ValueError):
        ops.edit_ops(a1[0], a1[1][:3], a1[2], a1[3])


def test_both_homes_of_the_move_bits(dev):
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    assert L.ctcn_edit_ops_ws_bytes(3, 1200, 300) > 0 and L.ctcn_edit_ops_ws_bytes(4, 40, 7) == 0
    rs = np.random.RandomState(4)
    _check(dev, _seqs(rs, [1200, 700, 3], 5), _seqs(rs, [300, 280, 300], 5), 1200, 300, V=5)           # workspace
    _check(dev, _seqs(rs, [40, 0, 17, 33], 5), _seqs(rs, [7, 7, 2, 0], 5), 40, 7, V=5)                 # LDS
    assert L.ctcn_edit_ops_ws_bytes(2, 4000, 64) > 0
    _check(dev, _seqs(rs, [4000, 3500], 5), _seqs(rs, [60, 64], 5), 4000, 64, class_map=[0, 1, 1, -1, 4], V=5)   # workspace, one column per lane


def test_longer_references_are_refused(dev):
    from ctc_pytorch_amd import ops
    args = _operands(dev, [[1, 2]], [[1] * 513], 2, 513)
    with pytest.raises(RuntimeError, match="512"):
        ops.edit_ops(*args)
    assert ops.edit_ops(*_operands(dev, [[1, 2]], [[1] * 512], 2, 512)).counts.cpu().tolist() == [[1, 510, 0, 1, 2, 512]]


def test_errors_equal_the_distance_kernel(dev):
    """Without a map sub + del + ins is ops.edit_distance on the same tensors, with `edit_wave` at its default."""
    from ctc_pytorch_amd import ops
    assert ops.get_option("edit_wave") == 1
    rs = np.random.RandomState(5)
    for lda, ldb in ((800, 50), (120, 200), (5, 1)):
        B = 32
        args = _operands(dev, _seqs(rs, rs.randint(0, lda + 1, B), 40), _seqs(rs, rs.randint(0, ldb + 1, B), 40), lda, ldb)
        c = ops.edit_ops(*args).counts
        assert torch.equal(c[:, :3].sum(1, dtype=torch.int32), ops.edit_distance(*args))
        assert torch.equal(c[:, 0] + c[:, 1] + c[:, 3], c[:, 5]) and torch.equal(c[:, 0] + c[:, 2] + c[:, 3], c[:, 4])


def test_decoders_and_model_score_like_the_host_path(dev, tmp_path):
    """Decoder.error_ops (both decoders; stats on the host, on the device, absent) and CTC_Model.compute_error_ops on a small synthetic
    model output: the totals and the table are the host alignment's of the ids the decoders return."""
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.utils import scoring
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder, GreedyDecoder
    T, B, V = 40, 5, 12
    b = synth.make_batch(seed=8, B=B, T=T, F=4, V=V, lab_lo=3, lab_hi=9)
    lp = torch.from_numpy(synth.make_logprobs(4, T, B, V, "peaky")).to(dev)
    lens, tl, tg = b["lens"].tolist(), b["tgt_len"], b["targets"]
    names = synth.int2char(V)
    cmap = np.arange(V, dtype=np.int32)
    cmap[3], cmap[5] = 2, -1
    arpa = str(tmp_path / "lm.arpa")
    synth.write_arpa(arpa, [names[i] for i in range(1, V)], seed=3, n_bigrams=30)
    greedy, beam = GreedyDecoder(names, space_idx=-1, blank_index=0), BeamDecoder(names, beam_width=5, blank_index=0, space_idx=-1, lm_path=arpa)
    hyp_ids = {greedy: greedy.decode_ids(lp, lens), beam: beam._decoder.decode_ids(lp, lens)[0]}
    flat = np.concatenate([tg[u, :tl[u]] for u in range(B)])
    for dec in (greedy, beam):
        for m in (None, cmap):
            want = scoring.ErrorStats(names)
            for u in range(B):
                want.add_pairs(*scoring.align_ids(hyp_ids[dec][u], tg[u, :tl[u]], m))
            tot = want.state()[:6].tolist()
            assert tot[5] > 0 and tot[3] > 0
            host, on_dev = scoring.ErrorStats(names), scoring.ErrorStats(names, device=dev)
            assert dec.error_ops(lp, lens, torch.from_numpy(tg), torch.from_numpy(tl), class_map=m) == tot
            assert dec.error_ops(lp, lens, torch.from_numpy(flat), tl.tolist(), class_map=m, stats=host) == tot      # the layout phone_word_error takes
            assert dec.error_ops(lp, lens, torch.from_numpy(tg), torch.from_numpy(tl), class_map=m, stats=on_dev).cpu().tolist() == tot
            assert torch.equal(host.state(), want.state()) and torch.equal(on_dev.state().cpu(), want.state())
            assert host.report() == want.report() == on_dev.report()
    rp = {"rnn_input_size": 4, "rnn_hidden_size": 8, "rnn_layers": 1, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": False}
    model = CTC_Model(rnn_param=rp, num_class=V, drop_out=0.0).to(dev)
    index = lp.argmax(-1).t().contiguous()
    for m in (None, cmap):
        want = np.sum([R.edit_ops(hyp_ids[greedy][u], tg[u, :tl[u]].tolist(), m)[0] for u in range(B)], axis=0).tolist()
        assert list(model.compute_error_ops(index, lens, tg, tl, class_map=m)) == want
    errs, tokens = model.compute_wer(index, lens, tg, tl)
    got = model.compute_error_ops(index.cpu().numpy(), np.asarray(lens), tg, tl)
    assert (got[0] + got[1] + got[2], got[5]) == (errs, tokens)


def test_run_epoch_validation_with_the_report(dev):
    """run_epoch(is_training=False, error_report=True): the same (1 - wer, loss) as without it, the same first line, one more line with
    the breakdown -- and under a score map total_wer and the return value are still those of the unmapped classes."""
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.steps.train_ctc import run_epoch
    from ctc_pytorch_amd.utils import scoring
    B, T, F, V = 4, 50, 8, 10
    rp = {"rnn_input_size": F, "rnn_hidden_size": 16, "rnn_layers": 1, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    m = CTC_Model(rnn_param=rp, num_class=V, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=21)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    m = m.to(dev)
    data = []
    for seed in (1, 2):
        z = synth.make_batch(seed=seed, B=B, T=T, F=F, V=V, lab_lo=3, lab_hi=8)
        data.append((torch.from_numpy(z["x"]), torch.from_numpy(z["frac"]), torch.from_numpy(z["targets"]), torch.from_numpy(z["tgt_len"]),
                     ["u%d" % u for u in range(B)]))
    loss_fn = nn.CTCLoss(reduction="sum")
    names = synth.int2char(V)
    cmap = np.arange(V, dtype=np.int32)
    cmap[4], cmap[6] = 3, -1
    plain, rep, mapped = [], [], []
    base = run_epoch(2, m, data, loss_fn, dev, is_training=False, log=plain.append)
    assert run_epoch(2, m, data, loss_fn, dev, is_training=False, log=rep.append, error_report=True, index2word=names) == base
    assert run_epoch(2, m, data, loss_fn, dev, is_training=False, log=mapped.append, error_report=True, score_map=cmap, index2word=names) == base
    assert len(plain) == 1 and rep[0] == plain[0] == mapped[0] and len(rep) == 2 and len(mapped) == 2
    # the breakdown against the host path on the model's own greedy ids
    with torch.no_grad():
        outs = [m(d[0].to(dev)) for d in data]
    for cm, line, tag in ((None, rep[1], ""), (cmap, mapped[1], " (mapped classes)")):
        want = scoring.ErrorStats(names)
        for d, out in zip(data, outs):
            lens = (d[1].numpy().astype(np.float32) * np.float32(out.shape[0])).astype(np.int64)
            for u, ids in enumerate(m_greedy(out, lens)):
                want.add_pairs(*scoring.align_ids(ids, d[2][u, :d[3][u]].numpy(), cm))
        assert line == "Epoch 2 Valid error breakdown%s: %s" % (tag, want.report().replace("\n", "; "))
    assert "%PER" in rep[1] and " ins, " in rep[1] and abs((1 - base[0]) * 100 - float(rep[1].split("%PER ")[1].split(" ")[0])) < 0.006


def m_greedy(out, lens):
    """Collapsed arg-max ids of (T, B, V) log-probs on the host: drop frame-to-frame repeats, then blanks (0)."""
    idx = out.argmax(-1).t().cpu().numpy()
    res = []
    for u in range(idx.shape[0]):
        row = idx[u, :lens[u]]
        res.append([int(k) for n, k in enumerate(row) if k != 0 and (n == 0 or k != row[n - 1])])
    return res
