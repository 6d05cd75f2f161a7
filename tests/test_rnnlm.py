"""GPU tests of the RNN language model: nn.Embedding / nn.CrossEntropyLoss, models/model_rnnlm.RNNLM against the torch-CPU oracle of
tests/lm_ref.py, steps/train_rnnlm on a Markov source, and n-best rescoring through utils/ctcDecoder.BeamDecoder."""
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as tnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_ref as R  # noqa: E402
from ctc_ref import log_softmax_bound  # noqa: E402
from ctc_pytorch_amd.testing import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def gates(prec, strict_act, strict_grad, strict_loss):
    return (strict_act, strict_grad, strict_loss) if prec == 0 else (1e-3, 1e-3, 1e-3)


def maxabs(a, b):
    a, b = (torch.as_tensor(t).detach().cpu().double() for t in (a, b))
    return float((a - b).abs().max()) if a.numel() else 0.0


def rel_l2(a, b):
    a, b = (torch.as_tensor(t).detach().cpu().double() for t in (a, b))
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_embedding_module_matches_torch_and_accumulates_in_flat_adam(dev):
    """nn.Embedding against torch.nn.Embedding on the CPU in float64: the forward is the same rows; the weight gradient is the ascending
    float32 sum, bit-equal to the restatement and within n (n - 1) u max|dy| of float64 per element (n - 1 additions of partial sums of at
    most n max|dy|, n = all positions).  In a FlatAdam the gradient lands in the flat buffer and a second backward pass doubles it exactly
    (fl(g + g) = 2 g); the padding row stays zero."""
    from ctc_pytorch_amd import nn, ops
    from ctc_pytorch_amd.optim import FlatAdam
    torch.manual_seed(2)
    V, E, pad = 13, 10, 4
    m = nn.Embedding(V, E, padding_idx=pad)
    ref = tnn.Embedding(V, E, padding_idx=pad).double()
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    m = m.to(dev)
    rng = np.random.RandomState(0)
    ids = rng.randint(0, V, size=(9, 7))
    ids[0, :3] = pad
    w = torch.from_numpy(rng.standard_normal((9, 7, E)).astype(np.float32))
    y = m(torch.from_numpy(ids).to(dev))
    yr = ref(torch.from_numpy(ids))
    assert torch.equal(y.detach().cpu().double(), yr.detach())
    (y * w.to(dev)).sum().backward()
    (yr * w.double()).sum().backward()
    want = R.embedding_bwd(ids, w.numpy().reshape(-1, E), np.zeros((V, E), np.float32), pad, 0.0)
    assert np.array_equal(m.weight.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    assert maxabs(m.weight.grad, ref.weight.grad) <= ids.size * (ids.size - 1) * R.U * float(w.abs().max())
    # a host id out of range is refused before upload; a device one gives zeros and raises where the caller synchronises
    with pytest.raises(ValueError):
        m(np.array([0, V]))
    bad = m(torch.tensor([1, V, 2], device=dev))
    assert not bad[1].any() and torch.equal(bad[0], m.weight[1]) and torch.equal(bad[2], m.weight[2])
    with pytest.raises(IndexError):
        ops.check_lm_status(dev)
    ops.check_lm_status(dev)                                             # (cleared by the raise)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.embed, self.fc = nn.Embedding(V, E, padding_idx=pad), nn.Linear(E, 5, bias=False)

        def forward(self, i):
            return self.fc(self.embed(i))
    net = Net().to(dev)
    opt = FlatAdam(net, lr=1e-3)
    opt.zero_grad()
    tid = torch.from_numpy(ids).to(dev)
    net(tid).sum().backward()
    assert net.embed.weight.grad.data_ptr() == net.embed.weight._ctcn_grad.data_ptr() and net.embed.weight.grad._base is opt.grad
    once = net.embed.weight.grad.clone()
    assert float(once.abs().sum()) > 0 and not once[pad].any() and float(net.fc.weight.grad.abs().sum()) > 0
    net(tid).sum().backward()
    assert torch.equal(net.embed.weight.grad, 2 * once)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_cross_entropy_module_matches_torch(dev, reduction):
    """nn.CrossEntropyLoss against torch.nn.CrossEntropyLoss on the CPU in float64.  Loss: per row within the log-softmax kernel's bound
    (tests/ctc_ref.log_softmax_bound), reductions within the sum of those plus one float32 rounding.  Gradient: against float64 on the
    kernel's own log-prob bits under tests/lm_ref.xent_bound, and against torch's float64 gradient under that bound widened by the
    log-softmax error carried through exp: |g_n| p expm1(bound_lp)."""
    from ctc_pytorch_amd import nn, ops
    rng = np.random.RandomState(3)
    N, V = 37, 29
    z = (rng.standard_normal((N, V)) * 3).astype(np.float32)
    tgt = rng.randint(0, V, size=N)
    tgt[[2, 11, 30]] = -7
    zd = torch.from_numpy(z).to(dev).requires_grad_(True)
    zr = torch.from_numpy(z).double().requires_grad_(True)
    loss = nn.CrossEntropyLoss(ignore_index=-7, reduction=reduction)(zd, torch.from_numpy(tgt).to(dev))
    want = tnn.CrossEntropyLoss(ignore_index=-7, reduction=reduction)(zr, torch.from_numpy(tgt))
    lsb = log_softmax_bound(z)
    row = np.where(tgt == -7, 0.0, lsb[np.arange(N), np.clip(tgt, 0, V - 1)])
    cnt = int((tgt != -7).sum())
    if reduction == "none":
        up = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
        assert loss.shape == (N,) and (np.abs(loss.detach().cpu().double().numpy() - want.detach().numpy()) <= row).all()
        assert not loss.detach().cpu()[[2, 11, 30]].any()
        (loss * up.to(dev)).sum().backward()
        (want * up.double()).sum().backward()
        g, stride, count = up.numpy(), 1, None
    else:
        scale = 1.0 if reduction == "sum" else 1.0 / cnt
        assert loss.dim() == 0 and abs(float(loss.detach()) - float(want.detach())) <= scale * row.sum() + 2 * R.U * abs(float(want.detach()))
        loss.backward()
        want.backward()
        g, stride, count = np.ones(1, np.float32), 0, (cnt if reduction == "mean" else None)
    lp = ops.log_softmax(torch.from_numpy(z).to(dev)).cpu().numpy()
    same, p, y, gn = R.xent_bwd(lp, tgt, g, stride, count, -7)
    bound = R.xent_bound(p, y, gn, reduction == "mean")
    got = zd.grad.cpu().double().numpy()
    assert (np.abs(got - same) <= bound).all()
    wide = bound + np.abs(gn)[:, None] * p * np.expm1(lsb) * (1 + 1e-3)
    assert (np.abs(got - zr.grad.numpy()) <= wide).all()
    assert not got[[2, 11, 30]].any()


# ---------------------------------------------------------------------------------------------------------------------------------
V, E, H, LAYERS = 11, 12, 16, 2
LABELLINGS = [[3, 4, 5, 3, 2, 9], [], [7, 7, 1], [2, 10, 4, 4, 8], [6, 1]]       # steps 7, 1, 4, 6, 3


def build(cell, bn, dev, seed=17):
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    m = RNNLM(V, emb_size=E, hidden_size=H, layers=LAYERS, rnn_type=getattr(nn, cell), batch_norm=bn, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=seed)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}
    m.load_state_dict(sd)
    ref = R.OracleRNNLM(V, E, H, LAYERS, getattr(tnn, cell), bn)
    ref.load_state_dict(sd)
    return m.to(dev), ref


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_model_parity_with_the_oracle(dev, cell, bn, prec):
    """Logits (max-abs), loss (relative) and every parameter gradient (rel-L2) against the torch-CPU oracle with the same state_dict on a
    ragged batch (sequences of 1 .. 7 steps), under the gates of test_model_three_steps_golden; three FlatAdam steps against
    torch.optim.Adam on the oracle under its loss gate; in evaluation mode score() against the oracle's float64 sum under the activation
    gate times the sequence length."""
    from ctc_pytorch_amd import ops
    from ctc_pytorch_amd.optim import FlatAdam
    ops.set_precision(prec)
    tol_act, tol_grad, tol_loss = gates(prec, 5e-5, 2e-4, 2e-5)
    m, ref = build(cell, bn, dev)
    m.train()
    ref.train()
    ids, tgt, lens = R.lm_batch(LABELLINGS)
    opt = FlatAdam(m, lr=1e-3, weight_decay=5e-4)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=5e-4)
    losses, losses_ref = [], []
    for step in range(3):
        if step == 0:
            with torch.no_grad():
                bn_state = {k: v.clone() for k, v in m.state_dict().items()}
                bn_state_ref = {k: v.clone() for k, v in ref.state_dict().items()}
                assert maxabs(m(ids, lens), ref(ids, lens)) < tol_act
            m.load_state_dict(bn_state)                              # (the extra forward moved the running statistics on both sides)
            ref.load_state_dict(bn_state_ref)
        loss = m.loss(LABELLINGS, reduction="mean")
        loss_ref = ref.loss(LABELLINGS, "mean")
        opt.zero_grad()
        opt_ref.zero_grad()
        loss.backward()
        loss_ref.backward()
        if step == 0:
            grads = dict(ref.named_parameters())
            for k, p in m.named_parameters():
                assert rel_l2(p.grad, grads[k].grad) < tol_grad or maxabs(p.grad, grads[k].grad) < 1e-6, k
        opt.step()
        opt_ref.step()
        losses.append(float(loss))
        losses_ref.append(float(loss_ref))
    assert np.allclose(losses, losses_ref, rtol=tol_loss), (losses, losses_ref)
    m.eval()
    ref64 = R.OracleRNNLM(V, E, H, LAYERS, getattr(tnn, cell), bn).double()
    ref64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    ref64.eval()
    got = m.score(LABELLINGS).cpu().numpy()
    want = ref64.score(LABELLINGS)
    assert got.dtype == np.float64 and (np.abs(got - want) <= tol_act * lens).all(), (got, want)
    ops.check_lm_status(dev)


def test_loss_reductions_and_padded_label_input(dev):
    """loss() takes padded (B, Lmax) labels with lengths as well as lists, and its reductions agree: sum = mean * tokens = the sum of
    'none'; the token losses behind a sequence are exact zeros."""
    m, _ = build("LSTM", True, dev)
    m.eval()
    Lmax = max(len(r) for r in LABELLINGS)
    padded = np.zeros((len(LABELLINGS), Lmax), dtype=np.int64)
    for b, r in enumerate(LABELLINGS):
        padded[b, :len(r)] = r
    n = [len(r) for r in LABELLINGS]
    with torch.no_grad():
        none = m.loss(LABELLINGS, reduction="none")
        total, mean = m.loss(torch.from_numpy(padded), torch.tensor(n), reduction="sum"), m.loss(padded, n, reduction="mean")
    tokens = sum(n) + len(n)
    assert none.shape == (Lmax + 1, len(n)) and abs(float(total) - float(none.double().sum())) <= 1e-5 * float(total)
    assert abs(float(mean) * tokens - float(total)) <= 1e-5 * float(total)
    _, tgt, _ = R.lm_batch(LABELLINGS)
    assert not none.cpu().numpy()[tgt == R.IGNORE].any()
    assert np.allclose(-m.score(LABELLINGS).cpu().numpy(), none.double().sum(0).cpu().numpy(), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_training_driver_learns_a_markov_source(dev, tmp_path):
    """steps/train_rnnlm.main on 300 sentences (12 .. 24 symbols) of a first-order Markov source over 8 classes whose successor has
    probability 0.85: conditional entropy 0.7146 nats, unigram entropy ln 8 = 2.0794, midpoint 1.3970.  The dev cross-entropy per token
    (60 sentences, boundary steps included) must end below the midpoint.  Sizes chosen on the torch-CPU oracle (tests/lm_ref.train_oracle,
    same batches, emb 8, hidden 16, 2 LSTM layers with BatchNorm, Adam lr 1e-2, batches of 30, 6 epochs): it reached
    2.096, 1.779, 1.341, 1.081, 0.994, 0.976 -- below the midpoint from the third epoch on, 0.42 nats of room at the end."""
    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    from ctc_pytorch_amd.steps import train_rnnlm
    P, cond, uni = R.markov_source()
    assert abs(uni - np.log(8)) < 1e-9 and 0.70 < cond < 0.73
    rng = np.random.RandomState(11)
    train, dev_set = R.sample_sentences(P, 300, rng), R.sample_sentences(P, 60, rng)
    out = str(tmp_path / "lm" / "rnnlm.pkl")
    lines = []
    conf = {"emb_size": 8, "hidden_size": 16, "layers": 2, "rnn_type": "LSTM", "batch_norm": True, "drop_out": 0.0, "batch_size": 30,
            "num_epoches": 6, "init_lr": 1e-2, "seed": 5, "output": out}
    model, hist = train_rnnlm.main(conf, train_sentences=train, dev_sentences=dev_set, num_class=9, log=lines.append)
    print("dev cross-entropy per epoch:", ["%.3f" % v for v in hist["dev_loss"]], "midpoint %.4f" % ((cond + uni) / 2))
    assert len(hist["dev_loss"]) == 6 and hist["best_dev_loss"] == min(hist["dev_loss"])
    assert hist["best_dev_loss"] < (cond + uni) / 2, hist["dev_loss"]
    assert hist["best_dev_loss"] > cond * 0.9                                        # (no model beats the source's entropy by much on 60 sentences)
    assert sum("dev_ppl" in l and l.startswith("Epoch") for l in lines) == 6
    back = RNNLM.load_package(out, dev)
    ce, tokens = train_rnnlm.evaluate(back, dev_set, 30)
    assert tokens == sum(len(s) + 1 for s in dev_set) and abs(ce - hist["best_dev_loss"]) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
T_, B_, VR = 40, 6, 12
LENS = [40, 33, 40, 28, 36, 40]


def competing_log_probs(seed):
    """(T, B, V) log-probs whose best labellings compete closely: segments of 4 frames, alternately blank and a phone; in every second
    phone segment two classes share the mass almost evenly (0.46 against 0.44), elsewhere the phone has 0.9."""
    rng = np.random.RandomState(seed)
    p = np.zeros((T_, B_, VR))
    for b in range(B_):
        for s in range(T_ // 4):
            rows = p[4 * s:4 * s + 4, b]
            rows[:] = rng.uniform(0.2, 1.0, size=(4, VR))
            rows /= rows.sum(-1, keepdims=True) / 0.1
            if s % 2 == 0:
                rows[:, 0] += 0.9
            else:
                c, c2 = rng.choice(np.arange(2, VR), size=2, replace=False)
                if (s // 2) % 2 == 0:
                    rows[:, c] += 0.46
                    rows[:, c2] += 0.44
                else:
                    rows[:, c] += 0.9
            rows /= rows.sum(-1, keepdims=True)
    return np.log(p).astype(np.float32)


@pytest.fixture(scope="module")
def rescoring(dev, tmp_path_factory):
    from ctc_pytorch_amd.models.model_rnnlm import RNNLM
    words = synth.int2char(VR)
    arpa = str(tmp_path_factory.mktemp("lm") / "lm.arpa")
    synth.write_arpa(arpa, [words[i] for i in range(1, VR)], seed=3, n_bigrams=40)
    torch.manual_seed(23)
    lm = RNNLM(VR, emb_size=8, hidden_size=16, layers=2, drop_out=0.0)
    vals = synth.fill_state_dict([(k, tuple(v.shape)) for k, v in lm.state_dict().items()], seed=29)
    lm.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})
    lm = lm.to(dev).eval()
    ref = R.OracleRNNLM(VR, 8, 16, 2, tnn.LSTM, True).double()
    ref.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in lm.state_dict().items()})
    ref.eval()
    lp = torch.from_numpy(competing_log_probs(4)).to(dev)
    return dict(words=words, arpa=arpa, lm=lm, ref=ref, lp=lp)


def decoder(c, **kw):
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    return BeamDecoder(c["words"], beam_width=20, blank_index=0, space_idx=-1, lm_path=c["arpa"], **kw)


def test_zero_weight_rescoring_is_the_plain_decoder_bit_for_bit(dev, rescoring):
    from ctc_pytorch_amd import ops
    c = rescoring
    plain, zero = decoder(c), decoder(c, rnnlm=c["lm"], rnnlm_weight=0.0, rnnlm_nbest=5, rnnlm_len_bonus=0.0)
    assert plain.decode(c["lp"], LENS) == zero.decode(c["lp"], LENS)
    assert plain.decode_async(c["lp"], LENS)() == zero.decode_async(c["lp"], LENS)()
    a, b = plain._device_ids(c["lp"], LENS), zero._device_ids(c["lp"], LENS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    d = plain._decoder
    _, _, score, _ = ops.beam_decode_device(c["lp"], LENS, d._lm_table_on(dev), d.lm_alpha, d.beamWidth, d.blank_index, False)
    best, status = zero._rescored(c["lp"], LENS)
    assert torch.equal(best.score.view(torch.int64), score.view(torch.int64)) and not best.k.any() and not status.any()
    assert int(a[1].min()) > 0


def test_rescoring_selects_what_the_restatement_selects_on_the_device_lm_scores(dev, rescoring):
    """Default weight: the device's LM scores meet the oracle's float64 sums under the activation gate times the sequence length, and
    best_k / ids / total are exactly the numpy select on the device's own LM scores (no near-tie can flake).  Weight 1e6: the winner is
    the entry the LM likes best, which is not entry 0 for at least one utterance."""
    from ctc_pytorch_amd import ops
    c = rescoring
    d = decoder(c, rnnlm=c["lm"], rnnlm_nbest=5)
    assert d.rnnlm_weight == 0.5 and d.rnnlm_len_bonus == 0.0
    s = d._decoder
    nb = ops.beam_decode_nbest_device(c["lp"], LENS, s._lm_table_on(dev), s.lm_alpha, s.beamWidth, 5, s.blank_index, False)
    out_ids, out_len, score, count, status = (t.cpu().numpy() for t in nb)
    assert not status.any() and count.min() >= 2
    for weight, bonus in ((0.5, 0.0), (0.5, 0.3), (1e6, 0.0)):
        d = decoder(c, rnnlm=c["lm"], rnnlm_nbest=5, rnnlm_weight=weight, rnnlm_len_bonus=bonus)
        best, st = d._rescored(c["lp"], LENS)
        lm = best.lm.cpu().numpy()
        labellings = [list(out_ids[b, k, :out_len[b, k]]) if k < count[b] else [] for b in range(B_) for k in range(5)]
        want_lm = c["ref"].score(labellings).reshape(B_, 5)
        steps = np.array([len(r) + 1 for r in labellings]).reshape(B_, 5)
        tol = 1e-3 if ops.get_precision() else 5e-5
        assert (np.abs(lm - want_lm) <= tol * steps).all()
        wi, wl, ws, wk = R.rescore_select(score, lm, out_len, count, out_ids, weight, bonus)
        assert np.array_equal(best.k.cpu().numpy(), wk) and np.array_equal(best.ids.cpu().numpy(), wi)
        assert np.array_equal(best.lengths.cpu().numpy(), wl) and np.array_equal(best.score.cpu().numpy().view(np.int64), ws.view(np.int64))
        ids, n, _ = d._device_ids(c["lp"], LENS)
        assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(n.cpu().numpy(), wl)
        if weight == 1e6:
            fav = np.array([int(np.argmax(lm[b, :count[b]])) for b in range(B_)])
            assert np.array_equal(wk, fav) and (fav != 0).any(), fav


def test_every_output_route_carries_the_rescored_hypothesis(dev, rescoring):
    """decode, decode_async, decode_timed, error_ops and the CTM writer all see the rescored winner; an utterance whose search reports a
    status yields the empty hypothesis and raises where the plain decoder raises."""
    from ctc_pytorch_amd.utils.ctm import write_ctm
    c = rescoring
    d = decoder(c, rnnlm=c["lm"], rnnlm_nbest=5, rnnlm_weight=1e6)
    plain = decoder(c)
    strings = d.decode(c["lp"], LENS)
    assert strings != plain.decode(c["lp"], LENS)                       # (the LM's favourite differs from the search's somewhere)
    ids, n, status = (t.cpu().numpy() for t in d._device_ids(c["lp"], LENS))
    assert strings == [" ".join(c["words"][k] for k in ids[b, :n[b]]) for b in range(B_)] == d.decode_async(c["lp"], LENS)()
    timed = d.decode_timed(c["lp"], LENS)
    assert all(e is not None for e in timed) and d.timed_strings(timed) == strings
    fh = io.StringIO()
    assert write_ctm(fh, ["u%d" % b for b in range(B_)], timed) == int(n.sum())
    assert [l.split()[4] for l in fh.getvalue().splitlines()] == " ".join(strings).split()
    targets = np.concatenate([ids[b, :n[b]] for b in range(B_)]).astype(np.int64)
    sub, dele, ins, cor, hyp_len, ref_len = d.error_ops(c["lp"], LENS, targets, n.tolist())
    assert (sub, dele, ins) == (0, 0, 0) and cor == hyp_len == ref_len == int(n.sum())
    short = [40, 33, 1] + LENS[3:]
    ids1, n1, status1 = (t.cpu().numpy() for t in d._device_ids(c["lp"], short))
    pst = plain._device_ids(c["lp"], short)[2].cpu().numpy()
    assert np.array_equal(status1, pst) and status1[2] != 0 and n1[2] == 0 and not ids1[2].any()
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(ids1[keep], ids[keep]) and np.array_equal(n1[keep], n[keep])
    for dec in (plain, d):
        with pytest.raises(IndexError):
            dec.decode(c["lp"], short)
    assert d.decode_timed(c["lp"], short)[2] is None
