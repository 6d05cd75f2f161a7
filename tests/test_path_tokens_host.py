"""Host-side checks of the timed, scored recognition output (no GPU): the entry point's declaration, the numpy restatement of its definition
(tests/path_tokens_ref.py) on hand-written cases, ops.path_tokens' argument errors, the CTM writer / reader, and the decode driver's `ctm` keys."""
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_tokens_ref as R  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import ctm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_resolves():
    header = open(os.path.join(ROOT, "include", "ctcn.h")).read()
    decl = re.search(r"int ctcn_path_tokens\(([^;]*)\);", header)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_lib._SIGS["ctcn_path_tokens"][1]) == 18
    fn = _lib.lib().ctcn_path_tokens
    assert fn.argtypes == _lib._SIGS["ctcn_path_tokens"][1]
    p = 64                                                              # a non-null stand-in: the argument checks come before any launch
    assert fn(None, 1, 1, p, p, p, p, p, p, p, p, p, p, 4, 2, 3, 0, None) == -1
    assert fn(p, 1, 1, p, p, p, p, p, p, p, p, p, p, 0, 2, 3, 0, None) == -1
    assert fn(p, 1, 1, p, p, p, p, p, p, p, p, p, p, 4, 2, 3, 3, None) == -1
    assert b"blank 3 outside [0, 3)" in _lib.lib().ctcn_last_error()


def _lp(T, V, seed=0):
    """(T, 1, V) log-probs whose entries are multiples of 1/8: every sum below is exact."""
    rs = np.random.RandomState(seed)
    return (-rs.randint(1, 64, size=(T, 1, V)) / 8.0).astype(np.float32)


def test_restatement_a_a_blank_a_gives_two_tokens():
    lp = _lp(4, 3)
    r = R.path_tokens([[1, 1, 0, 1]], [4], lp)
    assert r["lengths"].tolist() == [2] and r["ids"][0].tolist() == [1, 1, -1, -1]
    assert r["starts"][0].tolist() == [0, 3, -1, -1] and r["ends"][0].tolist() == [2, 4, -1, -1]
    assert r["mean_lp"][0, 0] == (lp[0, 0, 1] + lp[1, 0, 1]) / 2 and r["mean_lp"][0, 1] == lp[3, 0, 1]
    assert r["min_lp"][0, 0] == min(lp[0, 0, 1], lp[1, 0, 1]) and r["min_lp"][0, 1] == lp[3, 0, 1]
    lead = lambda t: lp[t, 0, 1] - max(lp[t, 0, 0], lp[t, 0, 2])
    assert r["mean_margin"][0, 0] == (lead(0) + lead(1)) / 2 and r["mean_margin"][0, 1] == lead(3)
    assert r["path_score"][0] == lp[0, 0, 1] + lp[1, 0, 1] + lp[2, 0, 0] + lp[3, 0, 1]
    assert (r["mean_lp"][0, 2:] == 0).all() and (r["min_lp"][0, 2:] == 0).all() and (r["mean_margin"][0, 2:] == 0).all()


def test_restatement_run_ending_at_n_and_frames_past_n_are_not_seen():
    lp = _lp(6, 4, seed=1)
    lp[4:] = np.nan                                                     # nothing at or past n is read
    r = R.path_tokens([[0, 2, 3, 3, 3, 1]], [4], lp)
    assert r["lengths"].tolist() == [2] and r["ids"][0, :2].tolist() == [2, 3]
    assert r["starts"][0, :2].tolist() == [1, 2] and r["ends"][0, :2].tolist() == [2, 4]
    assert r["path_score"][0] == lp[0, 0, 0] + lp[1, 0, 2] + lp[2, 0, 3] + lp[3, 0, 3]
    assert np.isfinite(r["mean_lp"]).all() and np.isfinite(r["mean_margin"]).all()
    over = R.path_tokens([[0, 2, 3, 3, 3, 1]], [9], _lp(6, 4, seed=1))  # lens beyond T is clamped to T
    assert over["lengths"].tolist() == [3] and over["ends"][0, :3].tolist() == [2, 5, 6]


def test_restatement_empty_all_blank_invalid_ids_and_a_moved_blank():
    lp = _lp(5, 3, seed=2)
    r = R.path_tokens([[1, 2, 1, 2, 1]], [0], lp)                       # n = 0
    assert r["lengths"].tolist() == [0] and r["path_score"].tolist() == [0.0] and (r["ids"] == -1).all() and (r["starts"] == -1).all()
    r = R.path_tokens([[1, 2, 1, 2, 1]], [-3], lp)                      # a negative length is n = 0
    assert r["lengths"].tolist() == [0] and r["path_score"].tolist() == [0.0]
    r = R.path_tokens([[0, 0, 0, 0, 0]], [5], lp)                       # all blank: no token, the score is still the path's
    assert r["lengths"].tolist() == [0] and r["path_score"][0] == lp[:, 0, 0].sum() and (r["ends"] == -1).all()
    r = R.path_tokens([[-1, 2, -1, 2, 7]], [5], lp)                     # -1 and 7 count as blank, never index lp, add 0
    assert r["lengths"].tolist() == [2] and r["starts"][0, :2].tolist() == [1, 3] and r["ends"][0, :2].tolist() == [2, 4]
    assert r["path_score"][0] == lp[1, 0, 2] + lp[3, 0, 2]
    r = R.path_tokens([[2, -1, 2, 2, -1]], [5], lp, blank=2)            # an invalid id between two blanks changes nothing
    assert r["lengths"].tolist() == [0] and r["path_score"][0] == lp[0, 0, 2] + lp[2, 0, 2] + lp[3, 0, 2]
    r = R.path_tokens([[0, 0, 2, 1, 1]], [5], lp, blank=2)              # blank 2: class 0 is a label like any other
    assert r["ids"][0, :2].tolist() == [0, 1] and r["starts"][0, :2].tolist() == [0, 3] and r["ends"][0, :2].tolist() == [2, 5]
    assert r["mean_margin"][0, 0] == ((lp[0, 0, 0] - max(lp[0, 0, 1], lp[0, 0, 2])) + (lp[1, 0, 0] - max(lp[1, 0, 1], lp[1, 0, 2]))) / 2
    one = R.path_tokens([[0, 0]], [2], _lp(2, 1))                       # V == 1: nothing but blank
    assert one["lengths"].tolist() == [0]


def test_path_tokens_argument_errors_come_before_the_device():
    T, B, V = 5, 2, 4
    lp, path, lens = torch.zeros(T, B, V), torch.zeros(T, B, dtype=torch.int32), [5, 3]
    for blank in (-1, V):
        with pytest.raises(ValueError, match="blank"):
            ops.path_tokens(path, lens, lp, blank=blank)
    with pytest.raises(ValueError, match="empty"):
        ops.path_tokens(torch.zeros(0, B, dtype=torch.int32), lens, torch.zeros(0, B, V))
    with pytest.raises(ValueError, match="empty"):
        ops.path_tokens(torch.zeros(T, 0, dtype=torch.int32), [], torch.zeros(T, 0, V))
    with pytest.raises(ValueError, match="does not match"):
        ops.path_tokens(path.t(), lens, lp)                             # (B, T) given as time-major
    with pytest.raises(ValueError, match="does not match"):
        ops.path_tokens(path, lens, lp, batch_major=True)
    with pytest.raises(ValueError, match="does not match"):
        ops.path_tokens(path[:4], lens, lp)
    with pytest.raises(ValueError, match="expected"):
        ops.path_tokens(path, lens, lp[0])
    with pytest.raises(ValueError, match="lengths"):
        ops.path_tokens(path, [5, 3, 1], lp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # well-formed arguments on the host: the device is the next thing asked for
        ops.path_tokens(path, lens, lp)


def test_ctm_round_trip_with_an_empty_utterance_and_a_missing_one():
    timed = [([("aa", 0, 3, 0.98765), ("b", 5, 6, 1.0)], -1.5), ([], -0.25), None, ([("sil", 12, 40, 0.5, -2.0, 0.75)], -3.0)]
    fh = io.StringIO()
    assert ctm.write_ctm(fh, ["u0", "u1", "u2", "u3"], timed, frame_shift=0.02, channel="A") == 3
    assert fh.getvalue() == "u0 A 0.000 0.060 aa 0.9877\nu0 A 0.100 0.020 b 1.0000\nu3 A 0.240 0.560 sil 0.5000\n"
    back = ctm.read_ctm(io.StringIO(fh.getvalue()))
    assert list(back) == ["u0", "u3"]                                   # given order; the empty and the missing utterance have no line
    assert back["u0"] == [("aa", 0.0, 0.06, 0.9877, "A"), ("b", 0.1, 0.02, 1.0, "A")] and back["u3"] == [("sil", 0.24, 0.56, 0.5, "A")]
    fh = io.StringIO()
    ctm.write_ctm(fh, ["z", "a"], [timed[3], timed[0]])                 # defaults: 10 ms frames, channel 1; no sorting
    assert [l.split()[:2] for l in fh.getvalue().splitlines()] == [["z", "1"], ["a", "1"], ["a", "1"]]
    assert ctm.read_ctm(io.StringIO(";; comment\n\nu 1 0.5 0.25 ah\n")) == {"u": [("ah", 0.5, 0.25, None, "1")]}
    with pytest.raises(ValueError):
        ctm.write_ctm(io.StringIO(), ["u0"], timed)
    with pytest.raises(ValueError):
        ctm.read_ctm(io.StringIO("u 1 0.5\n"))


def test_ctm_keys_default_off():
    import yaml
    from ctc_pytorch_amd.steps import decode_ctc
    from ctc_pytorch_amd.steps.train_ctc import Config
    assert decode_ctc.ctm_options(Config()) == {}
    for text, want in (("drop_out: 0.1", {}), ("ctm: null\nctm_frame_shift: 0.02", {}), ("ctm: ''", {}),
                       ("ctm: out.ctm", {"ctm": "out.ctm", "ctm_frame_shift": 0.01}),
                       ("ctm: out.ctm\nctm_frame_shift: 0.0125", {"ctm": "out.ctm", "ctm_frame_shift": 0.0125})):
        o = Config()
        for k, v in yaml.safe_load(text).items():
            setattr(o, k, v)
        assert decode_ctc.ctm_options(o) == want
    ap = decode_ctc.arg_parser()
    a = ap.parse_args(["--conf", "c.yaml"])
    assert a.ctm is None and a.ctm_frame_shift is None
    assert decode_ctc.apply_argv({"beam_width": 3}, a) == {"beam_width": 3}                       # no switch: the YAML as it is
    assert decode_ctc.apply_argv({"ctm": "y.ctm"}, a) == {"ctm": "y.ctm"}
    a = ap.parse_args(["--conf", "c.yaml", "--ctm", "x.ctm", "--ctm-frame-shift", "0.02"])
    assert decode_ctc.apply_argv({"ctm": "y.ctm"}, a) == {"ctm": "x.ctm", "ctm_frame_shift": 0.02}


class _StubModel(torch.nn.Module):
    def __init__(self, T, V):
        super().__init__()
        self.T, self.V = T, V

    def forward(self, x, *args, **kwargs):
        return torch.zeros(self.T, x.shape[0], self.V)


def test_decode_driver_with_ctm_scores_as_without_and_lists_the_utterances_in_loader_order(tmp_path):
    from ctc_pytorch_amd.steps import decode_ctc
    from ctc_pytorch_amd.utils.ctcDecoder import Decoder
    words = {0: "blank", 1: "aa", 2: "ao", 3: "b", 4: "q"}
    T, V = 8, 5
    strings = {2: [" aa b q", " ao"], 1: [" b b"]}
    spans = {2: [([("aa", 0, 2, 0.9), ("b", 2, 3, 0.8), ("q", 5, 8, 0.7)], -1.0), ([("ao", 1, 4, 0.6)], -2.0)], 1: [None]}
    calls = []

    class Dec(Decoder):
        def decode(self, probs, lens):
            return strings[probs.shape[1]]

        def decode_timed(self, probs, lens, frame_stride=1, detail=False):
            calls.append((probs.shape[1], list(lens), frame_stride))
            return [e if e is None else ([(p, s * frame_stride, t * frame_stride, c) for p, s, t, c in e[0]], e[1]) for e in spans[probs.shape[1]]]

    data = [(torch.zeros(2, T, V), torch.ones(2), torch.tensor([[2, 3, 0], [1, 3, 3]]), torch.tensor([2, 3]), ["spk2_u7", "spk1_u3"]),
            (torch.zeros(1, T, V), torch.ones(1), torch.tensor([[3, 3]]), torch.tensor([2]), ["spk0_u9"])]
    plain_log, log = [], []
    plain, dec = Dec(words, space_idx=-1), Dec(words, space_idx=-1)
    want = decode_ctc.decode_and_score(_StubModel(T, V), data, plain, words, "cpu", log=plain_log.append, mask_padding=False)
    assert calls == [] and list(tmp_path.iterdir()) == []               # off: no timed decode, no file
    out = str(tmp_path / "hyp.ctm")
    got = decode_ctc.decode_and_score(_StubModel(T, V), data, dec, words, "cpu", log=log.append, mask_padding=False, ctm=out,
                                      ctm_frame_shift=0.02, n_skip_frame=3)
    assert got == want and log == plain_log and len(log) == 2
    assert (dec.num_word, dec.num_char) == (plain.num_word, plain.num_char) and dec.num_word == 7
    assert calls == [(2, [T, T], 3), (1, [T], 3)]                       # the frames the decoder saw, the loader's frame skip as the stride
    assert open(out).read() == ("spk2_u7 1 0.000 0.120 aa 0.9000\nspk2_u7 1 0.120 0.060 b 0.8000\nspk2_u7 1 0.300 0.180 q 0.7000\n"
                                "spk1_u3 1 0.060 0.180 ao 0.6000\n")
    back = ctm.read_ctm(open(out))
    assert list(back) == ["spk2_u7", "spk1_u3"] and "spk0_u9" not in back
    # a rank of a sharded run names its file PATH.<rank> and pairs its k-th decode with minibatch rank + k * world
    name = decode_ctc.write_ctm_file(out, [["a"], ["b"], ["c"], ["d"]], [spans[1], [spans[2][1]]], 0.01, rank=1, world=2)
    assert name == out + ".1" and open(name).read() == "d 1 0.010 0.030 ao 0.6000\n"
    # with the error report on, the totals, the lines and the file are the same
    from ctc_pytorch_amd.utils import scoring
    log2, dec2, out2 = [], Dec(words, space_idx=-1), str(tmp_path / "hyp2.ctm")
    got2 = decode_ctc.decode_and_score(_StubModel(T, V), data, dec2, words, "cpu", log=log2.append, mask_padding=False,
                                       stats=scoring.ErrorStats(words), ctm=out2, ctm_frame_shift=0.02, n_skip_frame=3)
    assert got2 == want and log2[:2] == plain_log and open(out2).read() == open(out).read()


def test_input_frames_per_output_frame_follows_the_front_end_geometry():
    from ctc_pytorch_amd import nn
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    from ctc_pytorch_amd.steps import decode_ctc
    rp = {"rnn_input_size": 12, "rnn_hidden_size": 8, "rnn_layers": 1, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    assert decode_ctc.input_frames_per_output_frame(CTC_Model(rnn_param=rp, num_class=5, drop_out=0.0)) == 1
    layers = [[(1, 4), (3, 3), (1, 2), (1, 1), None], [(4, 4), (3, 3), (2, 2), (1, 1), (3, 1)]]
    m = CTC_Model(add_cnn=True, cnn_param={"batch_norm": True, "activate_function": nn.ReLU, "layer": layers}, rnn_param=rp, num_class=5, drop_out=0.0)
    assert decode_ctc.input_frames_per_output_frame(m) == 6             # time stride 1 * 2, time pooling 3
    n = np.array([600, 601, 1200])
    assert (np.abs(m.output_lengths(n).numpy() * 6 - n) <= 6 * 2).all()  # what output_lengths divides by, up to the kernels' edges
    assert decode_ctc.input_frames_per_output_frame(_StubModel(4, 3)) == 1
