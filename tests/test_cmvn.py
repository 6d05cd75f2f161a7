"""Per-speaker, per-utterance and sliding-window CMVN on the HIP kernels (ctcn_cmvn_accumulate_groups, ctcn_cmvn_apply, ctcn_cmvn_sliding)
through ops, utils/features.SpeakerCMVN / SlidingCMVN and steps/make_feat.py.  The demand is bit-identity with the numpy restatement of
tests/cmvn_ref.py (written from the contract in include/ctcn.h) and, for the sliding window, with the host twin as well.

Shapes: B = 6 with frames [0, 1, 63, 64, 65, 130] (an empty utterance, one row, one row short of a 64-row block, exactly one, one more, three
blocks) and F in {3, 81, 300} (300: the column loops beyond 256 threads); the sliding window with cmn_window 20 / min 5 on frames
[0, 1, 4, 5, 6, 20, 21, 22, 2 run + 3], run = the frames the kernel stages at a time, so that the longest utterance crosses two staging
boundaries with the window straddling each, and once at Kaldi's defaults on 650 frames.  Rows at or beyond an utterance's length hold NaN
and outputs are pre-filled with NaN: a read past the length or an element left unwritten shows."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cmvn_ref as R  # noqa: E402
from ctc_pytorch_amd import ops  # noqa: E402
from ctc_pytorch_amd.testing import synth  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402
from ctc_pytorch_amd.utils.data_loader import read_kaldi_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
FRAMES, TMAX, GROUPS, G = [0, 1, 63, 64, 65, 130], 130, [2, 0, 2, 1, 0, 2], 4
U32, U64 = 2.0 ** -24, 2.0 ** -53
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def batch(F):
    """(padded batch with NaN behind every utterance, pre-filled statistics, the restatement's statistics after the grouped call), once per F."""
    if F not in _CACHE:
        rs = np.random.RandomState(7 + F)
        x = np.full((len(FRAMES), TMAX, F), np.nan, dtype=np.float32)
        for b, n in enumerate(FRAMES):
            x[b, :n] = (2.0 * rs.standard_normal((n, F)) + 4.0 * rs.standard_normal(F)).astype(np.float32)
        pre = rs.standard_normal((G, 2, F + 1)) * 10.0
        _CACHE[F] = (x, pre, R.accumulate_groups(x, FRAMES, GROUPS, pre))
    return _CACHE[F]


@pytest.mark.parametrize("F", [3, 81, 300])
def test_grouped_accumulate(dev, F):
    x, pre, want = batch(F)
    xd, frames = torch.from_numpy(x).to(dev), torch.tensor(FRAMES, dtype=torch.int32, device=dev)
    stats = torch.from_numpy(pre).to(dev)
    assert ops.cmvn_accumulate_groups(xd, frames, GROUPS, stats) is stats
    got = stats.cpu().numpy()
    assert same(got[3], pre[3])                                        # nobody's group keeps its values exactly
    assert same(got, want)                                             # and the call ADDS, in the stated order
    assert not same(got[:3], pre[:3])
    # ids on the device are taken as they are; one outside [0, G) contributes nothing
    ids = torch.tensor([2, 0, 2, 1, 7, -1], dtype=torch.int32, device=dev)
    stats = torch.from_numpy(pre).to(dev)
    ops.cmvn_accumulate_groups(xd, frames, ids, stats)
    assert same(stats.cpu().numpy(), R.accumulate_groups(x, FRAMES, ids.tolist(), pre))
    # one group holding everybody: what ctcn_cmvn_accumulate writes
    one, ref = torch.from_numpy(pre[:1].copy()).to(dev), torch.from_numpy(pre[0].copy()).to(dev)
    ops.cmvn_accumulate_groups(xd, frames, [0] * len(FRAMES), one)
    ops.cmvn_accumulate(xd, frames, ref)
    assert same(one[0].cpu().numpy(), ref.cpu().numpy())
    assert same(one.cpu().numpy(), R.accumulate_groups(x, FRAMES, [0] * len(FRAMES), pre[:1]))
    assert same(ref.cpu().numpy(), R.accumulate_groups(x, FRAMES, [0] * len(FRAMES), pre[:1])[0])      # the global call itself, directly


@pytest.mark.parametrize("F", [3, 81, 300])
def test_apply(dev, F):
    x, _, stats = batch(F)
    stats = stats.copy()
    rs = np.random.RandomState(F)
    stats[3, 0, :F], stats[3, 1, :F], stats[3, 0, F] = rs.standard_normal(F) * 50, 400.0 + rs.uniform(0, 50, F), 20.0   # a fourth speaker, from elsewhere
    stats[1, 1, 0] = stats[1, 0, 0] ** 2 / stats[1, 0, F]               # a column without variance: the floor 1e-20
    xd, frames = torch.from_numpy(x).to(dev), torch.tensor(FRAMES, dtype=torch.int32, device=dev)
    sd = torch.from_numpy(stats).to(dev)
    # a single group
    for g in (0, 2):
        out = torch.full_like(xd, float("nan"))
        assert ops.cmvn_apply(xd, frames, sd[g], out=out) is out
        assert same(out.cpu().numpy(), R.apply(x, FRAMES, stats[g:g + 1]))
    # groups, both settings of norm_vars, zeros at and beyond each length
    for ids in (GROUPS, [3, 3, 1, 1, 0, 0]):
        for nv in (True, False):
            got = ops.cmvn_apply(xd, frames, sd, ids, norm_vars=nv, out=torch.full_like(xd, float("nan"))).cpu().numpy()
            assert same(got, R.apply(x, FRAMES, stats, ids, nv)), (ids, nv)
            for b, n in enumerate(FRAMES):
                assert not got[b, n:].any() and np.isfinite(got[b, :n]).all()
    # in place
    inplace = xd.clone()
    assert ops.cmvn_apply(inplace, frames, sd, GROUPS, out=inplace) is inplace
    assert same(inplace.cpu().numpy(), R.apply(x, FRAMES, stats, GROUPS))
    # an id outside [0, G) on the device, and a group without frames, copy the utterance through
    ids = torch.tensor([2, 0, 4, -1, 0, 2], dtype=torch.int32, device=dev)
    got = ops.cmvn_apply(xd, frames, sd, ids).cpu().numpy()
    assert same(got, R.apply(x, FRAMES, stats, ids.tolist())) and same(got[2, :63], x[2, :63]) and same(got[3, :64], x[3, :64])
    empty = stats.copy()
    empty[2] = 0.0
    got = ops.cmvn_apply(xd, frames, torch.from_numpy(empty).to(dev), GROUPS).cpu().numpy()
    assert same(got, R.apply(x, FRAMES, empty, GROUPS)) and same(got[5], np.nan_to_num(x[5], nan=0.0))
    with pytest.raises(ValueError, match="outside \\[0, 4\\)"):
        ops.cmvn_apply(xd, frames, sd, [0, 1, 2, 3, 4, 0])
    with pytest.raises(ValueError, match="outside \\[0, 4\\)"):
        ops.cmvn_accumulate_groups(xd, frames, [0, 1, 2, 3, -1, 0], sd)


def test_apply_with_one_group_is_the_fused_path(dev):
    cfg = features.FbankConfig(num_mel_bins=80, use_energy=True, dither=0.0)
    fb = features.Fbank(cfg, dev)
    waves = synth.make_waves(11, [4801, 9000, 1600, 7777])
    raw, frames = fb(waves)
    cmvn = features.GlobalCMVN(fb.feat_dim, dev).accumulate(raw, frames)
    mean, scale = cmvn.mean_scale(dev)
    fused, frames2 = fb(waves, mean=mean, scale=scale)
    assert torch.equal(frames, frames2)
    got = ops.cmvn_apply(raw, frames, cmvn.stats)
    assert same(got.cpu().numpy(), fused.cpu().numpy())
    spk = features.SpeakerCMVN(fb.feat_dim, ["all"], dev).accumulate(raw, frames, ["all"] * 4)
    assert torch.equal(spk.stats[0], cmvn.stats)
    assert same(spk.apply(raw, frames, ["all"] * 4).cpu().numpy(), fused.cpu().numpy())


def sliding_batch(F):
    key = ("sliding", F)
    if key not in _CACHE:
        run = ops.cmvn_sliding_run()
        frames = [0, 1, 4, 5, 6, 20, 21, 22, 2 * run + 3]
        rs = np.random.RandomState(31 + F)
        x = np.full((len(frames), frames[-1], F), np.nan, dtype=np.float32)
        for b, n in enumerate(frames):
            x[b, :n] = (2.0 * rs.standard_normal((n, F)) + 4.0 * rs.standard_normal(F)).astype(np.float32)
            x[b, :n, 1] = -7.5                                          # a constant column: the variance floor 1e-10, exact zeros
        _CACHE[key] = (x, frames)
    return _CACHE[key]


@pytest.mark.parametrize("F", [81, 300])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("nv", [False, True])
def test_sliding(dev, F, center, nv):
    x, frames = sliding_batch(F)
    assert frames[-1] > 2 * ops.cmvn_sliding_run() and 20 > ops.cmvn_sliding_run() // 2
    xd = torch.from_numpy(x).to(dev)
    out = torch.full_like(xd, float("nan"))
    assert ops.cmvn_sliding(xd, frames, 20, 5, nv, center, out=out) is out
    got = out.cpu().numpy()
    for b, n in enumerate(frames):
        want = R.sliding(x[b, :n], 20, 5, nv, center)
        assert same(got[b, :n], want), (b, n)
        assert same(got[b, :n], ops.cmvn_sliding_host(x[b, :n], 20, 5, nv, center))
        assert not got[b, n:].any() and not got[b, :n, 1].any()
    again = features.SlidingCMVN(20, 5, normalize_variance=nv, center=center)(xd, torch.tensor(frames, dtype=torch.int32, device=dev))
    assert same(again.cpu().numpy(), got)


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("nv", [False, True])
def test_sliding_at_kaldis_defaults(dev, center, nv):
    run = ops.cmvn_sliding_run()
    if "defaults" not in _CACHE:
        rs = np.random.RandomState(650)
        x = np.full((3, 650, 81), np.nan, dtype=np.float32)
        x[0] = (2.0 * rs.standard_normal((650, 81)) + 4.0 * rs.standard_normal(81)).astype(np.float32)
        x[1, :101] = x[0, :101] + np.float32(1.0)
        x[2, :3 * run + 9] = x[0, 200:200 + 3 * run + 9]                # an odd number of whole runs
        _CACHE["defaults"] = x
    x = _CACHE["defaults"]
    out = torch.full((3, 650, 81), float("nan"), device=dev)
    got = ops.cmvn_sliding(torch.from_numpy(x).to(dev), [650, 101, 3 * run + 9], normalize_variance=nv, center=center, out=out).cpu().numpy()
    for b, n in ((0, 650), (1, 101), (2, 3 * run + 9)):
        assert same(got[b, :n], R.sliding(x[b, :n], 600, 100, nv, center)), (b, n)
        assert same(got[b, :n], ops.cmvn_sliding_host(x[b, :n], normalize_variance=nv, center=center))
        assert not got[b, n:].any()


def test_sliding_refusals(dev):
    x = torch.zeros(2, 40, 8, device=dev)
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.cmvn_sliding(x, [40, 3], 20, 5, out=x)
    for win, minw in ((20, 21), (0, 0), (20, 0)):
        with pytest.raises(ValueError, match="cmn_window"):
            ops.cmvn_sliding(x, [40, 3], win, minw)


def _write_waves(tmp_path, lengths, seed):
    rs = np.random.RandomState(seed)
    waves, lines = [], []
    for i, n in enumerate(lengths):
        t = np.arange(n) / 16000.0
        w = 2000.0 * rs.standard_normal(n) * (0.3 + np.abs(np.sin(2 * np.pi * (1.0 + i) * t))) + 3000.0 * np.sin(2 * np.pi * (200.0 + 150.0 * i) * t)
        w = np.clip(np.round(w), -32768, 32767).astype(np.int16)
        path = str(tmp_path / ("utt%d.wav" % i))
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(w.astype("<i2").tobytes())
        waves.append(w)
        lines.append("utt%d %s\n" % (i, path))
    (tmp_path / "wav.scp").write_text("".join(lines))
    return waves


def test_make_feat_per_speaker_and_per_utterance(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    lengths = [9000, 4801, 16000, 7777, 12345, 5600]
    spk_of = ["sa", "sb", "sa", "sc", "sb", "sa"]
    waves = _write_waves(tmp_path, lengths, 78)
    (tmp_path / "fbank.conf").write_text("--num-mel-bins=40\n--dither=0\n")
    (tmp_path / "utt2spk").write_text("".join("utt%d %s\n" % (i, s) for i, s in enumerate(spk_of)))
    common = ["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp"), "--device", str(dev)]
    log = []
    out_dir = tmp_path / "spk"
    _, scp = make_feat.main(common + ["--out-dir", str(out_dir), "--utt2spk", str(tmp_path / "utt2spk")], log=log.append)
    assert sorted(os.listdir(str(out_dir))) == ["cmvn.ark.txt", "feats.ark", "feats.scp", "utt2spk"]
    assert open(str(out_dir / "utt2spk")).read() == open(str(tmp_path / "utt2spk")).read()
    entries = [l.split() for l in open(scp)]
    assert [e[0] for e in entries] == ["utt%d" % i for i in range(6)]
    mats = [read_kaldi_matrix(e[1]) for e in entries]
    # the Python API, in the driver's order (by length: the float64 sums are taken in batch order)
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf")), dev)
    order = sorted(range(6), key=lambda i: lengths[i])
    raw, frames = fb([waves[i] for i in order])
    cmvn = features.SpeakerCMVN(40, ["sa", "sb", "sc"], dev).accumulate(raw, frames, [spk_of[i] for i in order])
    normed = cmvn.apply(raw, frames, [spk_of[i] for i in order]).cpu().numpy()
    for j, i in enumerate(order):
        assert same(normed[j, :mats[i].shape[0]], mats[i]), i
    loaded = features.SpeakerCMVN.load_kaldi_text(str(out_dir / "cmvn.ark.txt"))
    assert loaded.speakers == ["sa", "sb", "sc"] and torch.equal(loaded.stats, cmvn.stats.cpu())
    # Per speaker and column, with m, s the exact mean and 1 / stddev of the raw values x_i and y_i = (x_i - m) s: the archive holds
    # fl32(fl32(x_i - fl32(m)) * fl32(s)) = y_i (1 + h_i) + c with |h_i| <= 3 u32 (1 + 3 u32) (one rounding per operation and that of s) and
    # |c| <= u32 |m| s (1 + 3 u32) (that of m).  mean(y) = 0 and mean(y^2) = 1, so |mean| <= 3 u32' mean|y| + |c| and
    # |mean square - 1| <= (2 h + h^2) + 2 |c| mean|y| (1 + h) + c^2; the statistics' own float64 error, (n + 8) u64 (sumsq / n) / var
    # relative, is added to both.
    rawh, nfr = raw.cpu().numpy().astype(np.float64), frames.cpu().numpy()
    for spk in ("sa", "sb", "sc"):
        x = np.concatenate([rawh[j, :nfr[j]] for j, i in enumerate(order) if spk_of[i] == spk])
        y = np.concatenate([mats[i] for i in range(6) if spk_of[i] == spk]).astype(np.float64)
        assert x.shape == y.shape
        m, var = x.mean(0), x.var(0)
        s = var ** -0.5
        ay = np.abs((x - m) * s).mean(0)
        h = 3 * U32 * (1 + 3 * U32)
        c = U32 * np.abs(m) * s * (1 + 3 * U32)
        e64 = (x.shape[0] + 8) * U64 * (x * x).mean(0) / var
        mean_bound = h * ay + c + e64
        sq_bound = 2 * h + h * h + 2 * c * ay * (1 + h) + c * c + 4 * e64
        print("%s: %d frames, max |mean| %.3g (bound %.3g), max |mean square - 1| %.3g (bound %.3g)"
              % (spk, x.shape[0], np.abs(y.mean(0)).max(), mean_bound.max(), np.abs((y * y).mean(0) - 1).max(), sq_bound.max()))
        assert (np.abs(y.mean(0)) <= mean_bound).all() and (np.abs((y * y).mean(0) - 1.0) <= sq_bound).all()
    # every utterance its own speaker: --cmvn-per-utt is --utt2spk with one speaker per utterance
    (tmp_path / "utt2utt").write_text("".join("utt%d utt%d\n" % (i, i) for i in range(6)))
    make_feat.main(common + ["--out-dir", str(tmp_path / "a"), "--utt2spk", str(tmp_path / "utt2utt"), "--norm-vars", "false"], log=log.append)
    make_feat.main(common + ["--out-dir", str(tmp_path / "b"), "--cmvn-per-utt", "--norm-vars", "false"], log=log.append)
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["cmvn.ark.txt", "feats.ark", "feats.scp"]
    assert open(str(tmp_path / "a" / "cmvn.ark.txt")).read() == open(str(tmp_path / "b" / "cmvn.ark.txt")).read()
    assert open(str(tmp_path / "a" / "feats.ark"), "rb").read() == open(str(tmp_path / "b" / "feats.ark"), "rb").read()
    per_utt = [read_kaldi_matrix(l.split()[1]) for l in open(str(tmp_path / "b" / "feats.scp"))]
    for j, i in enumerate(order):
        want = R.apply(raw[j:j + 1].cpu().numpy(), [int(nfr[j])], R.accumulate_groups(raw[j:j + 1].cpu().numpy(), [int(nfr[j])], [0], np.zeros((1, 2, 41))),
                       norm_vars=False)
        assert same(want[0, :nfr[j]], per_utt[i]), i
    # the sliding window, with deltas behind it
    make_feat.main(common + ["--out-dir", str(tmp_path / "s"), "--cmvn-sliding", "--cmn-window", "30", "--min-cmn-window", "10", "--cmn-center",
                             "--norm-vars", "true", "--delta-order", "1"], log=log.append)
    assert sorted(os.listdir(str(tmp_path / "s"))) == ["feats.ark", "feats.scp"]
    slid = [read_kaldi_matrix(l.split()[1]) for l in open(str(tmp_path / "s" / "feats.scp"))]
    want, wn, _ = features.FrameContext(delta_order=1)(features.SlidingCMVN(30, 10, True, True)(raw, frames), frames)
    for j, i in enumerate(order):
        assert same(want[j, :int(wn[j])].cpu().numpy(), slid[i]), i


def test_make_feat_copies_get_their_own_speaker_and_old_flags_their_old_output(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    lengths = [6000, 4801, 5600]
    waves = _write_waves(tmp_path, lengths, 79)
    (tmp_path / "fbank.conf").write_text("--num-mel-bins=40\n--dither=0\n")
    (tmp_path / "utt2spk").write_text("utt0 sa\nutt1 sb\nutt2 sa\n")
    common = ["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp"), "--device", str(dev)]
    log = []
    make_feat.main(common + ["--out-dir", str(tmp_path / "sp"), "--utt2spk", str(tmp_path / "utt2spk"), "--speed-perturb", "0.9,1.0"], log=log.append)
    assert open(str(tmp_path / "sp" / "utt2spk")).read() == ("sp0.9-utt0 sp0.9-sa\nsp1.0-utt0 sp1.0-sa\nsp0.9-utt1 sp0.9-sb\nsp1.0-utt1 sp1.0-sb\n"
                                                             "sp0.9-utt2 sp0.9-sa\nsp1.0-utt2 sp1.0-sa\n")
    stats = features.SpeakerCMVN.load_kaldi_text(str(tmp_path / "sp" / "cmvn.ark.txt"))
    assert stats.speakers == ["sp0.9-sa", "sp0.9-sb", "sp1.0-sa", "sp1.0-sb"]
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf")), dev)
    assert [int(v) for v in stats.stats[:, 0, 40]] == [sum(fb.num_frames(-(-lengths[i] * 10 // 9)) for i in (0, 2)), fb.num_frames(-(-lengths[1] * 10 // 9)),
                                                       sum(fb.num_frames(lengths[i]) for i in (0, 2)), fb.num_frames(lengths[1])]
    # none of the new flags: the archive of the global path, as before
    _, scp = make_feat.main(common + ["--out-dir", str(tmp_path / "g"), "--compute-cmvn"], log=log.append)
    assert sorted(os.listdir(str(tmp_path / "g"))) == ["feats.ark", "feats.scp", "global_fbank_cmvn.txt"]
    mats = [read_kaldi_matrix(l.split()[1]) for l in open(scp)]
    order = sorted(range(3), key=lambda i: lengths[i])
    raw, frames = fb([waves[i] for i in order])
    cmvn = features.GlobalCMVN(40, dev).accumulate(raw, frames)
    assert torch.equal(features.GlobalCMVN.load_kaldi_text(str(tmp_path / "g" / "global_fbank_cmvn.txt")).stats, cmvn.stats.cpu())
    mean, scale = cmvn.mean_scale()
    normed, _ = fb([waves[i] for i in order], mean=mean, scale=scale)
    for j, i in enumerate(order):
        assert same(normed[j, :mats[i].shape[0]].cpu().numpy(), mats[i]), i
    _, scp = make_feat.main(common + ["--out-dir", str(tmp_path / "r")], log=log.append)
    rawm = [read_kaldi_matrix(l.split()[1]) for l in open(scp)]
    for j, i in enumerate(order):
        assert same(raw[j, :rawm[i].shape[0]].cpu().numpy(), rawm[i]), i
