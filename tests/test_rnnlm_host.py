"""Host-side tests of the RNN language model (no GPU): refusals, package round trip, batch construction, the drivers' argv / YAML handling,
and the decode driver's unchanged default branch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_ref as R  # noqa: E402
from ctc_pytorch_amd.testing import synth  # noqa: E402


def test_modules_refuse_cpu_tensors_and_unsupported_arguments():
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nn.Embedding(5, 3)(torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nn.CrossEntropyLoss()(torch.zeros(2, 3), torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RNNLM(5, emb_size=4, hidden_size=4, layers=1)(np.zeros((3, 2), dtype=np.int64), [3, 2])
    for kw in ({"max_norm": 1.0}, {"sparse": True}, {"scale_grad_by_freq": True}):
        with pytest.raises(NotImplementedError):
            nn.Embedding(5, 3, **kw)(torch.tensor([1]))
    with pytest.raises(NotImplementedError):
        nn.CrossEntropyLoss(weight=torch.ones(3))
    with pytest.raises(NotImplementedError):
        nn.CrossEntropyLoss(label_smoothing=0.1)
    with pytest.raises(NotImplementedError):
        nn.CrossEntropyLoss()(torch.zeros(2, 3), torch.full((2, 3), 1.0 / 3))           # probability targets
    with pytest.raises(ValueError):
        nn.CrossEntropyLoss(reduction="batchmean")
    with pytest.raises(ValueError):
        RNNLM(1)


def test_host_ids_are_validated_before_upload():
    from ctc_pytorch_amd import ops
    ops.check_token_ids(np.array([0, 4, -100]), 5, "t", also=(-100,))
    with pytest.raises(ValueError, match="outside"):
        ops.check_token_ids(np.array([0, 5]), 5, "t")
    with pytest.raises(ValueError, match="outside"):
        ops.check_token_ids(np.array([0, -100]), 5, "t")
    with pytest.raises(ValueError):
        ops.token_ids(np.array([0.5]), 5, torch.device("cpu"))


@pytest.mark.parametrize("cell,bn", [("LSTM", True), ("GRU", False)])
def test_package_round_trip(tmp_path, cell, bn):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    torch.manual_seed(3)
    m = RNNLM(11, emb_size=12, hidden_size=16, layers=2, rnn_type=getattr(nn, cell), batch_norm=bn, drop_out=0.2)
    keys = list(m.state_dict())
    assert "embed.weight" in keys and "rnns.0.rnn.weight_ih_l0" in keys and "rnns.1.rnn.weight_hh_l0" in keys
    assert ("rnns.1.batch_norm.weight" in keys) == bn and ("fc.1.weight" in keys) == bn and ("fc.weight" in keys) == (not bn)
    assert not any("rnns.0.batch_norm" in k or "reverse" in k or "bias_" in k for k in keys)
    path = str(tmp_path / "rnnlm.pkl")
    torch.save(RNNLM.save_package(m, epoch=3, loss_results=[1.0], dev_loss_results=[2.0]), path)
    for source in (path, torch.load(path, weights_only=False)):
        back = RNNLM.load_package(source)
        assert (back.num_class, back.emb_size, back.hidden_size, back.layers, back.batch_norm, back.drop_out) == (11, 12, 16, 2, bn, 0.2)
        assert back.rnn_type is getattr(nn, cell)
        assert all(torch.equal(v, back.state_dict()[k]) for k, v in m.state_dict().items())
    # the oracle model of the tests shares the state_dict surface
    import torch.nn as tnn
    oracle = R.OracleRNNLM(11, 12, 16, 2, getattr(tnn, cell), bn)
    assert list(oracle.state_dict()) == keys
    oracle.load_state_dict(m.state_dict())


def test_batch_construction_boundary_ignore_and_length_sorting():
    from ctc_pytorch_amd.models import model_rnnlm as M
    rows = [[3, 4, 5], [], [7], [2, 2, 2, 2, 9]]
    ids, tgt, lens = M.lm_batch(rows)
    wi, wt, wl = R.lm_batch(rows)
    assert np.array_equal(ids, wi) and np.array_equal(tgt, wt) and np.array_equal(lens, wl)
    assert ids.shape == tgt.shape == (6, 4) and lens.tolist() == [4, 1, 2, 6]
    assert (ids[0] == M.BOUNDARY).all() and M.BOUNDARY == 0 and M.IGNORE == -100
    assert ids[:, 0].tolist() == [0, 3, 4, 5, 0, 0] and tgt[:, 0].tolist() == [3, 4, 5, 0, -100, -100]
    assert ids[:, 1].tolist() == [0] * 6 and tgt[:, 1].tolist() == [0] + [-100] * 5
    # the device pack kernel's rule is the same one (its restatement, on an n-best list of these rows)
    out_ids = np.zeros((2, 2, 5), dtype=np.int32)
    for s, r in enumerate(rows):
        out_ids[s // 2, s % 2, :len(r)] = r
    pi, pt, pl = R.pack_nbest(out_ids, np.array([[3, 0], [1, 5]], dtype=np.int32), np.array([2, 2], dtype=np.int32), 5)
    assert np.array_equal(pi, ids) and np.array_equal(pt, tgt) and np.array_equal(pl, lens)
    rng = np.random.RandomState(0)
    sents = [list(rng.randint(2, 9, size=n)) for n in rng.randint(0, 12, size=37)]
    plain = M.length_sorted_batches(sents, 8)
    assert sorted(i for b in plain for i in b) == list(range(37)) and [len(b) for b in plain] == [8, 8, 8, 8, 5]
    flat = [len(sents[i]) for b in plain for i in b]
    assert flat == sorted(flat)
    mixed = M.length_sorted_batches(sents, 8, shuffle_seed=5)
    assert sorted(map(tuple, mixed)) == sorted(map(tuple, plain)) and mixed != plain
    assert mixed == M.length_sorted_batches(sents, 8, shuffle_seed=5)


def test_train_driver_argv_and_yaml_handling(tmp_path):
    from ctc_pytorch_amd.steps import train_rnnlm as T
    from ctc_pytorch_amd.utils.data_loader import Vocab
    a = T.arg_parser().parse_args(["--epochs", "3", "--init-lr", "0.01", "--no-batch-norm", "--output", "x.pkl", "--rnn-type", "GRU"])
    conf = T.apply_argv({"num_epoches": 9, "hidden_size": 64, "batch_norm": True, "seed": 7}, a)
    assert conf == {"num_epoches": 3, "hidden_size": 64, "batch_norm": False, "seed": 7, "init_lr": 0.01, "output": "x.pkl", "rnn_type": "GRU"}
    opts = T.options(conf)
    assert opts["emb_size"] == 128 and opts["layers"] == 2 and opts["lr_decay"] == 0.5 and opts["max_grad_norm"] is None and opts["num_epoches"] == 3
    assert T.apply_argv({"seed": 7}, T.arg_parser().parse_args([])) == {"seed": 7}          # no switch: the YAML's keys alone
    with pytest.raises(ValueError, match="unknown keys"):
        T.options({"hiden_size": 3})
    with pytest.raises(ValueError):
        T.options({"max_grad_norm": 0.0})
    with pytest.raises(ValueError):
        T.options({"lr_decay": 1.5})
    units = tmp_path / "units"
    units.write_text("aa\nbb\ncc\n")
    lab = tmp_path / "lab"
    lab.write_text("u1 aa bb cc\nu2 cc zz\nu3\nu4 bb\n")
    assert T.read_labels(str(lab), Vocab(str(units))) == [[2, 3, 4], [4, 1], [3]]            # zz -> UNK; the empty utterance is dropped


def test_decode_driver_keys_and_unchanged_default_branch(monkeypatch):
    from ctc_pytorch_amd.steps import decode_ctc, test_ctc
    from ctc_pytorch_amd.steps.train_ctc import Config
    ap = decode_ctc.arg_parser()
    conf = decode_ctc.apply_argv({"rnnlm_weight": 0.2, "beam_width": 8}, ap.parse_args(["--rnnlm-path", "lm.pkl", "--rnnlm-nbest", "5", "--rnnlm-len-bonus", "0.1"]))
    assert conf == {"rnnlm_weight": 0.2, "beam_width": 8, "rnnlm_path": "lm.pkl", "rnnlm_nbest": 5, "rnnlm_len_bonus": 0.1}
    assert decode_ctc.apply_argv({"beam_width": 8}, ap.parse_args([])) == {"beam_width": 8}
    opts = Config()
    assert decode_ctc.rnnlm_options(opts) == {}
    for k, v in conf.items():
        setattr(opts, k, v)
    assert decode_ctc.rnnlm_options(opts) == {"rnnlm": "lm.pkl", "rnnlm_weight": 0.2, "rnnlm_nbest": 5, "rnnlm_len_bonus": 0.1}
    opts.rnnlm_nbest = 0
    with pytest.raises(ValueError):
        decode_ctc.rnnlm_options(opts)
    opts.rnnlm_nbest, opts.decode_type = 5, "Greedy"
    with pytest.raises(ValueError, match="Greedy"):
        decode_ctc.make_decoder(opts, synth.int2char(9))
    # none of the new keys: decode_ctc.main is test_ctc.main, as before; with rnnlm_path it is not
    calls = []
    monkeypatch.setattr(test_ctc, "main", lambda conf, **kw: calls.append(conf) or ("CER", "WER"))
    base = {"decode_type": "Beam", "beam_width": 8, "use_gpu": False}
    assert decode_ctc.main(dict(base)) == ("CER", "WER") and calls == [base]
    assert decode_ctc.main(dict(base, rnnlm_path=None, rnnlm_weight=0.7)) == ("CER", "WER") and len(calls) == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_ctc.main(dict(base, rnnlm_path="lm.pkl"))
    assert len(calls) == 2


def test_beam_decoder_clamps_nbest_to_the_beam_width_and_keeps_its_default_path(tmp_path):
    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    V = 9
    words = synth.int2char(V)
    arpa = str(tmp_path / "lm.arpa")
    synth.write_arpa(arpa, [words[i] for i in range(1, V)], seed=3, n_bigrams=30)
    lm = RNNLM(V, emb_size=4, hidden_size=4, layers=1)
    assert BeamDecoder(words, beam_width=4, lm_path=arpa, rnnlm=lm, rnnlm_nbest=10).rnnlm_nbest == 4
    assert BeamDecoder(words, beam_width=20, lm_path=arpa, rnnlm=lm).rnnlm_nbest == 10
    path = str(tmp_path / "rnnlm.pkl")
    torch.save(RNNLM.save_package(lm), path)
    d = BeamDecoder(words, beam_width=20, lm_path=arpa, rnnlm=path, rnnlm_weight=0.25, rnnlm_nbest=3, rnnlm_len_bonus=0.5)
    assert isinstance(d.rnnlm, RNNLM) and (d.rnnlm_weight, d.rnnlm_nbest, d.rnnlm_len_bonus) == (0.25, 3, 0.5)
    assert BeamDecoder(words, beam_width=20, lm_path=arpa).rnnlm is None
    with pytest.raises(ValueError):
        BeamDecoder(words, beam_width=20, lm_path=arpa, rnnlm=RNNLM(V + 1, emb_size=4, hidden_size=4, layers=1))
    with pytest.raises(ValueError):
        BeamDecoder(words, beam_width=20, lm_path=arpa, rnnlm=lm, rnnlm_nbest=0)


def test_restatement_agrees_with_torch_on_the_cpu():
    """tests/lm_ref.py against torch's own CPU kernels where torch defines the same thing: embedding backward (index_add into zeros, float64,
    to rounding), NLL and the cross-entropy gradient."""
    import torch.nn.functional as F
    rng = np.random.RandomState(1)
    N, V, E = 50, 7, 5
    ids = rng.randint(0, V, size=N)
    dy = rng.standard_normal((N, E)).astype(np.float32)
    want = torch.zeros(V, E, dtype=torch.float64).index_add_(0, torch.from_numpy(ids), torch.from_numpy(dy).double()).numpy()
    got = R.embedding_bwd(ids, dy, np.zeros((V, E), np.float32))
    assert np.allclose(got, want, rtol=0, atol=N * R.U * np.abs(dy).max() * 4)
    assert np.array_equal(R.embedding_bwd(ids, dy, np.ones((V, E), np.float32), beta=1.0, padding_idx=2)[2], np.ones(E, np.float32))
    z = torch.from_numpy(rng.standard_normal((12, V)).astype(np.float32))
    tgt = rng.randint(0, V, size=12)
    tgt[3] = R.IGNORE
    lp = torch.log_softmax(z, -1).numpy()
    tok, seq, total, count, status = R.nll(lp, tgt, 4, 3)
    want_tok = F.nll_loss(torch.from_numpy(lp), torch.from_numpy(tgt), ignore_index=R.IGNORE, reduction="none").numpy()
    assert np.array_equal(tok, want_tok) and count == 11 and status == 0 and abs(total - want_tok.astype(np.float64).sum()) < 1e-12
    assert np.allclose(seq, want_tok.reshape(4, 3).astype(np.float64).sum(0), rtol=0, atol=1e-12)
    zz = z.double().requires_grad_(True)
    F.cross_entropy(zz, torch.from_numpy(tgt), ignore_index=R.IGNORE, reduction="mean").backward()
    dz, p, y, gn = R.xent_bwd(lp, tgt, np.array([1.0], np.float32), 0, count=11)
    assert np.allclose(dz, zz.grad.numpy(), rtol=0, atol=1e-6)
    assert (R.xent_bound(p, y, gn, True) > 0).all()
