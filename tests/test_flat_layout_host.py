"""Host tests of optim.flat_layout, the device-free layout arithmetic of optim.FlatAdam: every parameter starts on a multiple of 4 elements
(16 bytes), and a model whose sizes are all multiples of 4 -- every shipped and golden configuration -- keeps the unpadded layout."""
import json
import os

import numpy as np
import pytest

from ctc_pytorch_amd import nn
from ctc_pytorch_amd.models.model_ctc import CTC_Model
from ctc_pytorch_amd.optim import ALIGN, flat_layout, placement_order

G = os.path.join(os.path.dirname(__file__), "golden")
CNN32 = [[(1, 32), (3, 3), (1, 2), (1, 1), None], [(32, 32), (3, 3), (2, 2), (1, 1), None]]


def _placed_sizes(model):
    named = [(n, p.numel()) for n, p in model.named_parameters() if p.requires_grad]
    order = placement_order([n for n, _ in named])
    return [named[i][0] for i in order], [named[i][1] for i in order]


def _prefix_sums(sizes):
    return [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])], int(np.sum(sizes))


def _model(F=40, H=16, L=2, rnn="LSTM", V=62, layers=None, bi=True, bn=True):
    rp = {"rnn_input_size": F, "rnn_hidden_size": H, "rnn_layers": L, "rnn_type": getattr(nn, rnn), "bidirectional": bi, "batch_norm": bn}
    if layers is None:
        return CTC_Model(rnn_param=rp, num_class=V, drop_out=0.0)
    return CTC_Model(add_cnn=True, cnn_param={"batch_norm": True, "activate_function": nn.ReLU, "layer": layers}, rnn_param=rp, num_class=V, drop_out=0.0)


def _shipped():
    shapes = json.load(open(os.path.join(G, "large_checksums.json")))
    out = {"cfg1": dict(V=62, H=128, L=2, rnn="LSTM", cnn=False)}
    for k in ("cfg2", "cfg3", "cfg4", "ref_yaml"):
        out[k] = shapes[k]["shape"]
    return out


GOLDEN_FAMILIES = {
    "lstm2x32": dict(H=32), "gru2x24": dict(H=24, rnn="GRU"), "rnn2x20_uni_nobn": dict(H=20, rnn="RNN", bi=False, bn=False),
    "cnn_lstm2x16": dict(layers=CNN32), "cnn_pool_lstm2x16": dict(layers=[[(1, 8), (3, 3), (1, 2), (1, 1), (2, 1)], [(8, 8), (3, 3), (1, 2), (1, 1), (3, 1)]]),
    "cnn_bigbank_lstm2x16": dict(F=121, layers=[[(1, 32), (3, 41), (1, 2), (0, 0), None], [(32, 32), (3, 21), (2, 2), (0, 0), None]]),
}


def test_flat_layout_random_sizes_start_on_16_bytes():
    rs = np.random.RandomState(0)
    for trial in range(200):
        sizes = [int(s) for s in rs.randint(1, 70, size=rs.randint(1, 30))]
        if trial % 4 == 0:
            sizes = [4 * s for s in sizes]
        offs, total = flat_layout(sizes)
        assert all(o % ALIGN == 0 for o in offs)
        ends = [o + n for o, n in zip(offs, sizes)]
        assert offs[0] == 0 and total == ends[-1]
        assert all(0 <= b - a < ALIGN for a, b in zip(ends, offs[1:])), "in order, no overlap, less than one quad of padding"
        if trial % 4 == 0:
            assert (offs, total) == _prefix_sums(sizes)


@pytest.mark.parametrize("which", ["odd_cnn", "odd_input"])
def test_flat_layout_of_the_odd_sized_models(which):
    odd = [[(1, 3), (3, 3), (1, 2), (1, 1), None], [(3, 5), (3, 3), (1, 2), (1, 1), None]]
    m = _model(V=13, layers=odd) if which == "odd_cnn" else _model(F=39, V=13)
    names, sizes = _placed_sizes(m)
    plain = dict(zip(names, _prefix_sums(sizes)[0]))
    if which == "odd_cnn":                     # what the unpadded layout was: W_hh of the first layer 2 floats off a 16-byte boundary
        assert (plain["conv.0.conv.bias"], plain["conv.0.batch_norm.weight"], plain["conv.0.batch_norm.bias"]) == (27, 30, 33)
        assert plain["rnns.0.rnn.weight_ih_l0"] == 186 and plain["rnns.0.rnn.weight_hh_l0"] % 4 == 2
    offs, total = flat_layout(sizes)
    at = dict(zip(names, offs))
    assert all(o % 4 == 0 for o in offs)
    if which == "odd_cnn":
        assert total > sum(sizes)
    else:                                      # 39 inputs: odd leading dimensions, but every size a multiple of 4
        assert (offs, total) == _prefix_sums(sizes)
    for n, size in zip(names, sizes):          # the two W_ih of a layer stay one (2*G*H, I) matrix where G*H*I is a multiple of 4
        if n.endswith("weight_ih_l0") and size % 4 == 0 and n + "_reverse" in at:
            assert at[n + "_reverse"] == at[n] + size, n


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "ref_yaml"] + sorted(GOLDEN_FAMILIES))
def test_flat_layout_of_shipped_and_golden_models_is_the_unpadded_one(name):
    if name in GOLDEN_FAMILIES:
        m = _model(**GOLDEN_FAMILIES[name])
    else:
        c = _shipped()[name]
        m = _model(F=c.get("F", 40), H=c["H"], L=c["L"], rnn=c["rnn"], V=c["V"], layers=CNN32 if c["cnn"] else None)
    _, sizes = _placed_sizes(m)
    assert all(s % 4 == 0 for s in sizes)
    assert flat_layout(sizes) == _prefix_sums(sizes)


def test_flat_gradient_is_found_across_alignment_padding():
    """nn.utils.clip_grad_norm_ looks for the one flat gradient behind a parameter list (nn._flat_grad_of): views laid out by flat_layout tile
    it but for the alignment padding, which must not send the call to torch's per-tensor path; a missing view or a real gap still does."""
    import torch
    sizes = [27, 3, 3, 3, 135, 5, 64]
    offs, total = flat_layout(sizes)
    assert any(b - (a + n) > 0 for a, n, b in zip(offs, sizes, offs[1:]))
    flat = torch.zeros(total)
    ps = []
    for o, n in zip(offs, sizes):
        p = torch.nn.Parameter(torch.zeros(n))
        p._ctcn_grad = flat[o:o + n]
        ps.append(p)
    found = nn._flat_grad_of(ps)
    assert found is not None and found.data_ptr() == flat.data_ptr() and found.numel() == total
    assert nn._flat_grad_of(ps[:4] + ps[5:]) is None            # a parameter missing: a gap of 135 elements
    assert nn._flat_grad_of(ps[:-1]) is None                    # the tail is not covered
