"""Per-speaker, per-utterance and sliding-window CMVN, the host side, without a GPU: the window rule (ctcn_cmvn_sliding_window) against the
restatement of tests/cmvn_ref.py and its own properties; the sliding host twin (ctcn_cmvn_sliding_host, the kernel's arithmetic) bit for
bit against the restatement, within a derived bound of the restatement in Kaldi's arithmetic and of a direct float64 mean and variance
over every window; ctcn_cmvn_norm_host against GlobalCMVN.mean_scale; the text archive, utt2spk, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmvn_ref as R  # noqa: E402
from ctc_pytorch_amd import ops  # noqa: E402
from ctc_pytorch_amd.steps import make_feat  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

U32 = 2.0 ** -24          # unit roundoff of float32
U64 = 2.0 ** -53          # and of float64
SMALL = [((7, 3), range(0, 71)), ((7, 7), range(0, 71)), ((1, 1), range(0, 71)), ((600, 100), (99, 100, 101, 600, 601, 650))]


def test_window_rule_and_its_properties():
    for (win, minw), lengths in SMALL:
        for center in (False, True):
            for n in lengths:
                ps = pe = None
                for t in range(n):
                    s, e = ops.cmvn_sliding_window(t, n, win, minw, center)
                    assert (s, e) == R.window(t, n, win, minw, center), (win, minw, center, n, t)
                    assert 0 <= s < e <= n
                    # The issue states e - s <= max(cmn_window, min_cmn_window).  Under the rule it also states (Kaldi's), a frame at or past
                    # cmn_window without `center` has s = t - cmn_window, e = t + 1: cmn_window + 1 frames.  The bound below is the rule's own:
                    # the issue's where it holds (centred), one frame more where the rule gives one frame more.
                    assert e - s <= (win if center else max(win + 1, minw))
                    if center:
                        assert e - s <= max(win, minw)
                    if ps is not None:
                        assert 0 <= s - ps <= 1 and 0 <= e - pe <= 1
                    if not center or n >= win:
                        assert s <= t < e
                    ps, pe = s, e


def _data(n, F, seed):
    rs = np.random.RandomState(seed)
    return (3.0 * rs.standard_normal((n, F)) + 5.0 * rs.standard_normal(F)).astype(np.float32)


CASES = [(n, w, c, nv) for n in (0, 1, 4, 5, 6, 20, 21, 22, 70) for w in ((20, 5), (7, 7), (1, 1)) for c in (False, True) for nv in (False, True)] + \
        [(650, (600, 100), c, nv) for c in (False, True) for nv in (False, True)]


def test_sliding_twin_equals_the_restatement_bit_for_bit():
    for k, (n, (win, minw), center, nv) in enumerate(CASES):
        x = _data(n, 5, k)
        padded = np.concatenate([x, np.full((3, 5), np.nan, np.float32)])           # NaN behind the length: never read
        got = ops.cmvn_sliding_host(padded[:n], win, minw, nv, center)
        want = R.sliding(x, win, minw, nv, center)
        assert got.dtype == np.float32 and got.shape == (n, 5)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, win, minw, center, nv)
    x = np.full((30, 2), 3.25, np.float32)                                          # a constant column: variance floor 1e-10, exact zeros
    assert not ops.cmvn_sliding_host(x, 20, 5, True, False).any()


def _window_moments(x, win, minw, center):
    """Direct float64 mean and variance (ddof 0) of every frame's window, and the window sizes."""
    n = x.shape[0]
    xd = x.astype(np.float64)
    m, v, w = np.zeros(x.shape), np.zeros(x.shape), np.zeros(n, np.int64)
    for t in range(n):
        s, e = R.window(t, n, win, minw, center)
        m[t], v[t], w[t] = np.mean(xd[s:e], axis=0), np.var(xd[s:e], axis=0), e - s
    return xd, m, v, w


def test_sliding_twin_against_kaldis_form():
    """Means only, both outputs are ONE float32 rounding of a double: the twin's of d = x - S / w, Kaldi's of x + a S with a = fl32(-1 / w)
    = -(1 + r) / w, |r| <= u32, i.e. of d - r m.  So |twin - kaldi| <= u32 |m| + u32 (|d| + |d - r m|) (+ the float64 roundings inside
    either, a factor 1 + 1e-6 covers them).  With the variance, Kaldi rounds d to float32 first and the product again; the two factors
    differ by the float64 roundings of the two variance forms, Q / w - m^2 against Q / w - S^2 / w^2: each is a difference of two terms
    of size Q / w and m^2 carrying a few roundings, so |v_t - v_k| <= 8 u64 (Q / w + m^2), and the factor v^-0.5 moves by half that
    relative to v, plus the roundings of sqrt, the division and pow: rho = 4 u64 (Q / w + m^2) / v + 8 u64."""
    for k, (n, (win, minw), center, nv) in enumerate(CASES):
        if n == 0:
            continue
        x = _data(n, 5, 100 + k)
        got = ops.cmvn_sliding_host(x, win, minw, nv, center).astype(np.float64)
        kaldi = R.sliding_kaldi(x, win, minw, nv, center).astype(np.float64)
        xd, m, v, w = _window_moments(x, win, minw, center)
        d = xd - m
        if not nv:
            bound = (U32 * np.abs(m) + U32 * (2 * np.abs(d) + U32 * np.abs(m))) * (1 + 1e-6) + 1e-300
        else:
            q = v + m * m                                                           # Q / w
            one = (w <= 1)[:, None]
            vf = np.where(one, 1.0, np.maximum(v, 1e-10))
            isd = vf ** -0.5
            rho = np.where(one, 0.0, 4 * U64 * (q + m * m) / vf + 8 * U64)
            d_k = np.abs(d) + U32 * np.abs(m)                                       # |d - r m|
            # twin: one rounding of d isd; Kaldi: fl32(fl32(d - r m) isd_k): two roundings
            bound = (isd * (U32 * np.abs(m) + U32 * np.abs(d) + 2 * U32 * d_k * (1 + U32)) + np.abs(d) * isd * rho) * (1 + 1e-6) + 1e-300
        err = np.abs(got - kaldi)
        assert (err <= bound).all(), (n, win, minw, center, nv, float((err / bound).max()))


def test_sliding_twin_against_a_direct_mean_and_variance():
    """Ties the restatement to the definition.  The running sum S_t has gone through at most w_0 + 2 t float64 additions and subtractions
    of values below X = max |x|, every intermediate below W X (W the largest window): |S_t - exact| <= (w_0 + 2 t) u64 W X, and the same
    for Q with X^2.  numpy's own mean over w values errs by at most w u64 X.  Hence E_m, the distance of the twin's mean from np.mean; the
    means-only output is one float32 rounding of x - m: |out - (x - mean)| <= u32 |x - mean| + E_m (1 + u32).  With the variance:
    v = Q / w - m^2 is off by at most E_Q / w + (2 |m| + E_m) E_m + 4 u64 (Q / w + m^2) from the exact value, np.var by at most
    (w + 4) u64 of its own; s = v^-0.5 then moves by at most E_v / 2 (v - E_v)^-1.5 (mean value theorem) plus three roundings, and
    out = fl32(d s)."""
    for k, (n, (win, minw), center, nv) in enumerate(c for c in CASES if c[0] >= 20 and c[1] != (1, 1)):
        x = _data(n, 5, 200 + k)
        got = ops.cmvn_sliding_host(x, win, minw, nv, center).astype(np.float64)
        xd, m, v, w = _window_moments(x, win, minw, center)
        X, W, wf = np.abs(xd).max(), w.max(), w[:, None].astype(np.float64)
        ops_done = (w[0] + 2 * np.arange(n))[:, None].astype(np.float64)
        E_S, E_Q = ops_done * U64 * W * X, ops_done * U64 * W * X * X
        E_m = E_S / wf + (wf + 2) * U64 * X
        d = xd - m
        if not nv:
            want, bound = d, U32 * np.abs(d) + E_m * (1 + U32)
        else:
            q = v + m * m
            E_v = E_Q / wf + (2 * np.abs(m) + E_m) * E_m + 4 * U64 * (q + m * m) + (wf + 4) * U64 * v
            assert (E_v < v / 2).all() and (v > 1e-10).all()                        # random data: far from the floor
            s = v ** -0.5
            E_s = 0.5 * E_v * (v - E_v) ** -1.5 + 4 * U64 * s
            want = d * s
            exact = (np.abs(d) + E_m) * (s + E_s) - np.abs(d) * s                   # |(d + dd)(s + ds) - d s|
            bound = U32 * (np.abs(want) + exact) + exact
        err = np.abs(got - want)
        assert (err <= bound * (1 + 1e-6)).all(), (n, win, minw, center, nv, float((err / bound).max()))
        if not nv:                                                                  # and the bound is the float32 rounding, not the slack
            assert (bound <= 1.001 * U32 * np.abs(d) + 1e-9).all()


def test_mean_and_scale_are_global_cmvns():
    rs = np.random.RandomState(5)
    F, n = 9, 37
    x = (2.0 * rs.standard_normal((n, F)) + 3.0).astype(np.float32).astype(np.float64)
    x[:, 4] = 1.5                                                                    # zero variance: the floor 1e-20
    c = features.GlobalCMVN(F)
    c.stats[0, :F] = torch.from_numpy(x.sum(0))
    c.stats[1, :F] = torch.from_numpy((x * x).sum(0))
    c.stats[0, F] = n
    mean, scale = c.mean_scale()
    got_m, got_s = ops.cmvn_norm_host(c.stats.numpy())
    assert np.array_equal(got_m.view(np.uint32), mean.view(np.uint32)) and np.array_equal(got_s.view(np.uint32), scale.view(np.uint32))
    assert got_s[4] == np.float32(1e10)
    rm, rscale = R.mean_scale(c.stats.numpy())
    assert np.array_equal(rm, mean) and np.array_equal(rscale, scale)
    got_m, got_s = ops.cmvn_norm_host(c.stats.numpy(), norm_vars=False)
    assert np.array_equal(got_m, mean) and np.array_equal(got_s, np.ones(F, np.float32))
    with pytest.raises(RuntimeError, match="no frames"):
        ops.cmvn_norm_host(np.zeros((2, F + 1)))


def test_text_archive_and_utt2spk(tmp_path):
    rs = np.random.RandomState(6)
    c = features.SpeakerCMVN(4, ["fadg0", "sp0.9-fadg0", "mbdg0"])
    c.stats.copy_(torch.from_numpy(rs.standard_normal((3, 2, 5)) * 1e3))
    p = str(tmp_path / "cmvn.ark.txt")
    c.save_kaldi_text(p)
    text = open(p).read()
    assert text.startswith("fadg0  [\n  ") and text.count("]\n") == 3 and "%.17g " % c.stats[0, 0, 0].item() in text
    back = features.SpeakerCMVN.load_kaldi_text(p)
    assert back.speakers == c.speakers and back.feat_dim == 4 and torch.equal(back.stats, c.stats)
    # Kaldi's own writer: fewer digits, the first row on the key's line is accepted too
    (tmp_path / "kaldi.txt").write_text("a  [\n  1 2 3 \n  4 5 0 ]\nb  [ 1.5 2 3\n 4 5 0 ]\n")
    k = features.SpeakerCMVN.load_kaldi_text(str(tmp_path / "kaldi.txt"))
    assert k.speakers == ["a", "b"] and k.stats.tolist() == [[[1, 2, 3], [4, 5, 0]], [[1.5, 2, 3], [4, 5, 0]]]
    (tmp_path / "bad.txt").write_text("a  [\n  1 2 3 \n")
    with pytest.raises(ValueError, match="not a Kaldi text archive"):
        features.SpeakerCMVN.load_kaldi_text(str(tmp_path / "bad.txt"))
    with pytest.raises(ValueError, match="every name once"):
        features.SpeakerCMVN(4, ["a", "a"])
    with pytest.raises(ValueError, match="unknown speaker"):
        c._ids(["fadg0", "nobody"])
    (tmp_path / "utt2spk").write_text("fadg0_sa1 fadg0\nfadg0_sa2 fadg0\n\nmbdg0_si833 mbdg0\n")
    assert features.read_utt2spk(str(tmp_path / "utt2spk")) == {"fadg0_sa1": "fadg0", "fadg0_sa2": "fadg0", "mbdg0_si833": "mbdg0"}
    (tmp_path / "utt2spk").write_text("fadg0_sa1 fadg0\nfadg0_sa2\n")
    with pytest.raises(ValueError, match="utt2spk:2: expected"):
        features.read_utt2spk(str(tmp_path / "utt2spk"))
    (tmp_path / "utt2spk").write_text("u a\nu b\n")
    with pytest.raises(ValueError, match="given twice"):
        features.read_utt2spk(str(tmp_path / "utt2spk"))
    keys = ["u1", "rev1-u1", "sp0.9-u2", "rev1-sp0.9-u2"]
    assert make_feat.copy_speakers(keys, ["u1", "u1", "u2", "u2"], {"u1": "a", "u2": "b"}) == ["a", "rev1-a", "sp0.9-b", "rev1-sp0.9-b"]
    assert make_feat.copy_speakers(keys, ["u1", "u1", "u2", "u2"], None) == keys
    with pytest.raises(ValueError, match="no speaker for u2"):
        make_feat.copy_speakers(keys, ["u1", "u1", "u2", "u2"], {"u1": "a"})


def test_refusals(tmp_path):
    x = np.zeros((12, 3), np.float32)
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.cmvn_sliding_host(x, 7, 3, out=x)
    buf = np.zeros((13, 3), np.float32)
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.cmvn_sliding_host(buf[:12], 7, 3, out=buf[1:])
    for win, minw in ((7, 8), (0, 0), (0, 1), (7, 0)):
        with pytest.raises(RuntimeError, match="cmn_window"):
            ops.cmvn_sliding_host(x, win, minw)
        with pytest.raises(RuntimeError, match="cmn_window"):
            ops.cmvn_sliding_window(0, 5, win, minw)
        with pytest.raises(ValueError, match="cmn_window"):
            features.SlidingCMVN(win, minw)
    with pytest.raises(RuntimeError, match="frame 5 of 5"):
        ops.cmvn_sliding_window(5, 5, 7, 3)
    # the device entry points check their arguments before they need the device
    feats, frames = torch.zeros(2, 4, 3), [4, 2]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cmvn_sliding(feats, frames)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cmvn_apply(feats, frames, torch.zeros(1, 2, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cmvn_accumulate_groups(feats, frames, [0, 0], torch.zeros(1, 2, 4, dtype=torch.float64))
    for ids in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="outside \\[0, 2\\)"):
            ops._cmvn_groups("cmvn_apply", ids, 2, 2, torch.device("cpu"))
    with pytest.raises(ValueError, match="3 group ids for a batch of 2"):
        ops._cmvn_groups("cmvn_apply", [0, 1, 1], 2, 2, torch.device("cpu"))
    with pytest.raises(ValueError, match="expected feats"):
        ops.cmvn_sliding(torch.zeros(4, 3), [4])
    # the driver: one normalisation per archive
    common = ["--conf", str(tmp_path / "none.conf"), "--wav-scp", str(tmp_path / "none.scp"), "--out-dir", str(tmp_path / "out")]
    u2s = ["--utt2spk", str(tmp_path / "utt2spk")]
    for extra, what in ((u2s + ["--cmvn-per-utt"], "exclude each other"), (u2s + ["--cmvn-sliding"], "exclude each other"),
                        (u2s + ["--compute-cmvn"], "exclude each other"), (["--cmvn-per-utt", "--cmvn-sliding"], "exclude each other"),
                        (["--cmvn-per-utt", "--compute-cmvn"], "exclude each other"), (["--cmvn-sliding", "--compute-cmvn"], "exclude each other"),
                        (["--cmvn-sliding", "--cmvn-stats", "x"], "keeps no statistics"), (["--cmn-window", "300"], "belongs to --cmvn-sliding"),
                        (["--min-cmn-window", "50"], "belongs to --cmvn-sliding"), (["--cmn-center"], "belongs to --cmvn-sliding"),
                        (["--norm-vars", "false"], "--norm-vars belongs"), (["--compute-cmvn", "--norm-vars", "true"], "--norm-vars belongs"),
                        (["--cmvn-sliding", "--cmn-window", "50"], "--min-cmn-window 1 to --cmn-window"),
                        (["--cmvn-sliding", "--cmn-window", "0", "--min-cmn-window", "0"], "at least 1"),
                        (["--feat-type", "logspec"] + u2s, "every utterance"), (["--feat-type", "logspec", "--cmvn-per-utt"], "every utterance"),
                        (["--feat-type", "logspec", "--cmvn-sliding"], "every utterance"), (["--feat-type", "logspec", "--norm-vars", "true"], "every utterance")):
        with pytest.raises(ValueError, match=what):
            make_feat.parse_args(common + extra)
        with pytest.raises(ValueError, match=what):
            make_feat.main(common + extra)
    assert not (tmp_path / "out").exists()
    a = make_feat.parse_args(common + ["--cmvn-sliding"])
    assert (a.cmn_window, a.min_cmn_window, a.cmn_center, a.norm_vars) == (600, 100, False, False)
    assert make_feat.parse_args(common + u2s).norm_vars is True and make_feat.parse_args(common + ["--cmvn-per-utt", "--norm-vars", "false"]).norm_vars is False
    assert make_feat.parse_args(common + ["--cmvn-sliding", "--norm-vars", "true", "--cmn-center"]).norm_vars is True
