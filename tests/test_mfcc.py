"""The MFCC front-end on the HIP kernel (ctcn_mfcc through its C entry point, ops.mfcc, utils/features.Mfcc, steps/make_feat.py --feat-type
mfcc) against the filterbank kernel it shares stages 1-4 with and against the numpy restatement of Kaldi's algorithm in tests/mfcc_ref.py.

Two bounds.
Pinned to the filterbank kernel: ctcn_fbank gives the kernel's own float32 log-mel rows m; steps 2-5 of the restatement in float64 on those
rows give c.  The kernel's value must lie within (N + 3) eps32 |L_k| sum_n |D[k][n] m[n]| of c (eps32 = 2^-23, L_k the lifter, which is
negative for k between Q and 2 Q: 64 cepstra under the default Q = 22 get there): the worst case
of an N-term float32 dot product with once-rounded coefficients and one more multiplication (one more factor (1 + eps32) sqrt 2 for HTK's
C0).  The energy column is the filterbank's bit for bit.  A wrong normaliser, row, column rule or lifter moves values by units; the bound
is 2e-3 .. 4e-2 on values of tens.
End to end, the rule of tests/test_fbank.py: e32 = the largest difference of the float32 and float64 restatements on the batch; the
kernel within max(4 e32, 1e-5) of the float64 one.  Every test prints its figures before it asserts; the measured ones are in DESIGN.md
section 7j."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfcc_ref as MR  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402
from ctc_pytorch_amd.utils.data_loader import read_kaldi_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def make_signals():
    """The six utterances of the filterbank's parity batches as float32 on Kaldi's scale, from one seeded generator: no frame, one sample
    short of a frame, exactly one frame, a partial workgroup, many workgroups with a ragged last one; and one of 561 samples."""
    rs = np.random.RandomState(20240)
    t = np.arange(16037) / 16000.0
    sig = [np.zeros(0),
           3000.0 * rs.standard_normal(399),                                           # noise of sigma 3000
           8000.0 * np.sin(2 * np.pi * 1000.0 * t[:400] + 0.3),                        # a tone alone
           6000.0 * np.sin(2 * np.pi * 440.0 * t[:1360]) + 50.0 * rs.standard_normal(1360),
           np.round(3000.0 * rs.standard_normal(16037)),                               # integer samples, as read from a file
           3000.0 * rs.standard_normal(561)]
    return [s.astype(np.float32) for s in sig]


SIGNALS = make_signals()
BATCHES = (SIGNALS[:5], SIGNALS[5:])
CONFIGS = {
    "kaldi_defaults": dict(),
    "shipped": dict(use_energy=False),                                  # the reference's conf/mfcc.conf
    "40bins_20ceps": dict(num_mel_bins=40, num_ceps=20, window_type="hamming"),
    "80bins_64ceps_no_lifter": dict(num_mel_bins=80, num_ceps=64, cepstral_lifter=0.0),      # all 64 lanes own a coefficient, N a multiple of 64
    "23ceps": dict(num_ceps=23),                                        # C == N
    "htk_compat": dict(htk_compat=True),
    "htk_compat_c0": dict(htk_compat=True, use_energy=False),
    "energy_after_window": dict(raw_energy=False),
    "energy_floor": dict(energy_floor=3.6e9),                           # 400 samples of sigma 3000: about half the frames lie below
    "reflected_edges": dict(snip_edges=False),
    "8khz": dict(sample_frequency=8000.0),                              # Npad 256
    "50ms_128bins_64ceps": dict(frame_length=50.0, num_mel_bins=128, num_ceps=64),           # Npad 1024: the largest LDS footprint
}
_REF, _RUN = {}, {}


def reference(name, bi):
    """[(float64 MFCCs, float32 MFCCs)] per utterance of a batch; computed once per configuration and shared."""
    k = (name, bi)
    if k not in _REF:
        o = MR.options(dither=0.0, **CONFIGS[name])
        _REF[k] = [(MR.mfcc(s, o, np.float64), MR.mfcc(s, o, np.float32)) for s in BATCHES[bi]]
    return _REF[k]


def pad(signals, dtype=np.float32, extra=0, fill=0):
    out = np.full((len(signals), max(max(s.shape[0] for s in signals), 1) + extra), fill, dtype=dtype)
    for b, s in enumerate(signals):
        out[b, :s.shape[0]] = s
    return out


def run_raw(fe, batch, lens, dev, extra_rows=3, mean=None, scale=None, dither=0.0, seed=0, utt_offset=0):
    """ctcn_mfcc (fe a features.Mfcc) or ctcn_fbank (a features.Fbank) called directly, outputs pre-filled with a sentinel, `extra_rows`
    rows more than any utterance needs."""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    entry = _lib.lib().ctcn_mfcc if isinstance(fe, features.Mfcc) else _lib.lib().ctcn_fbank
    w = torch.from_numpy(batch).to(dev)
    B, Nmax = batch.shape
    Tmax = max(fe.num_frames(n) for n in lens) + extra_rows
    feats = torch.full((B, Tmax, fe.feat_dim), SENTINEL, dtype=torch.float32, device=dev)
    frames = torch.full((B,), -7777, dtype=torch.int32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    _lib.check(entry(p(w), int(batch.dtype == np.int16), p(lens_d), ctypes.byref(fe.plan.opts), p(fe.plan.on(dev)), p(mean), p(scale),
                     p(feats), p(frames), B, Nmax, Tmax, float(dither), seed, utt_offset, _lib.stream_ptr()), "front-end")
    return feats.cpu().numpy(), frames.cpu().numpy()


def check_rows(feats, frames, lens, fe):
    """frames exact, every element written, every row at or beyond frames[b] exactly zero."""
    assert frames.tolist() == [fe.num_frames(n) for n in lens], (frames, lens)
    assert not (feats == SENTINEL).any()
    for b, n in enumerate(frames):
        assert not feats[b, n:].any(), (b, n)


def fbank_of(kw):
    """The filterbank configuration that shares the MFCC configuration's stages 1-4."""
    o = MR.fbank_options(MR.options(dither=0.0, **kw))
    return features.FbankConfig(**o)


def outputs(dev, name, bi):
    """(MFCC front-end, its raw output, its frames, the filterbank kernel's raw output) of a batch; run once per configuration and shared."""
    k = (name, bi)
    if k not in _RUN:
        kw = CONFIGS[name]
        mf = features.Mfcc(features.MfccConfig(dither=0.0, **kw), dev)
        fb = features.Fbank(fbank_of(kw), dev)
        signals = BATCHES[bi]
        lens = [s.shape[0] for s in signals]
        fb_feats, fb_frames = run_raw(fb, pad(signals), lens, dev)
        feats, frames = run_raw(mf, pad(signals), lens, dev)
        check_rows(feats, frames, lens, mf)
        assert np.array_equal(frames, fb_frames)
        _RUN[k] = (mf, feats, frames, fb_feats)
    return _RUN[k]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pinned_to_the_filterbank_kernel(dev, name):
    kw = CONFIGS[name]
    o = MR.options(dither=0.0, **kw)
    N, C = o["num_mel_bins"], o["num_ceps"]
    D, lift = MR.dct_matrix(N, C), MR.lifter(C, float(np.float32(o["cepstral_lifter"])))
    worst, rows = 0.0, 0
    for bi in range(len(BATCHES)):
        mf, feats, frames, fb_feats = outputs(dev, name, bi)
        assert feats.shape[2] == C
        for b, n in enumerate(frames):
            if n == 0:
                continue
            m32, e32 = MR.split_fbank(fb_feats[b, :n], o)
            m = np.ascontiguousarray(m32).astype(np.float64)
            want = MR.cepstra(m, None if e32 is None else e32.astype(np.float64), o, np.float64)
            bound = (N + 3) * EPS32 * np.abs(lift)[None, :] * (np.abs(m)[:, None, :] * np.abs(D)[None, :, :]).sum(axis=2)
            got = feats[b, :n]
            if o["use_energy"]:
                ecol = C - 1 if o["htk_compat"] else 0
                assert np.array_equal(got[:, ecol], e32), (name, bi, b)                  # the filterbank's energy column, bit for bit
                bound[:, 0] = 0.0
            elif o["htk_compat"]:
                bound[:, 0] *= (1.0 + EPS32) * np.sqrt(2.0)
            if o["htk_compat"]:
                bound = MR.htk_order(bound)
            err = np.abs(got.astype(np.float64) - want)
            mask = bound > 0
            worst = max(worst, float((err[mask] / bound[mask]).max()))
            rows += int(n)
            assert (err <= bound).all(), (name, bi, b, float((err - bound).max()))
        if name == "energy_floor" and bi == 0:
            r64 = reference(name, 0)[4][0]
            floor = np.log(np.float64(np.float32(3.6e9)))
            assert (r64[:, 0] == floor).any() and (r64[:, 0] > floor).any()            # the floor bites on some frames only
    print("%s: largest |kernel - float64 steps 2-5 on the kernel's log-mels| / bound = %.3g over %d frames" % (name, worst, rows))
    assert rows > 0 and worst <= 1.0


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_parity_with_the_restatement(dev, name):
    for bi, signals in enumerate(BATCHES):
        mf, feats, frames, _ = outputs(dev, name, bi)
        ref = reference(name, bi)
        e32 = ek = 0.0
        for b, (r64, r32) in enumerate(ref):
            assert r64.shape == (frames[b], mf.feat_dim)
            if not r64.size:
                continue
            e32 = max(e32, float(np.abs(r32.astype(np.float64) - r64).max()))
            ek = max(ek, float(np.abs(feats[b, :frames[b]].astype(np.float64) - r64).max()))
        print("%s batch %d: e32 %.3g, kernel %.3g, bound %.3g" % (name, bi, e32, ek, max(4 * e32, 1e-5)))
        assert ek <= max(4.0 * e32, 1e-5), (name, bi, ek, e32)
        if bi == 0:                                                     # the Python surface gives the same bits, without the spare rows
            f2, n2 = mf(signals)
            assert np.array_equal(n2.cpu().numpy(), frames) and np.array_equal(f2.cpu().numpy(), feats[:, :f2.shape[1]])


def test_batch_invariance_and_input_types(dev):
    mf = features.Mfcc(features.MfccConfig(dither=0.0), dev)
    ints = [np.clip(np.round(s), -32768, 32767) for s in SIGNALS[:5]]
    lens = [s.shape[0] for s in ints]
    as_f32, frames = run_raw(mf, pad(ints), lens, dev)
    check_rows(as_f32, frames, lens, mf)
    assert frames.tolist() == [0, 0, 1, 7, 98] and as_f32.shape[2] == 13
    as_i16, frames_i = run_raw(mf, pad(ints, np.int16), lens, dev)
    assert np.array_equal(frames, frames_i) and np.array_equal(as_f32, as_i16)
    wide, frames_w = run_raw(mf, pad(ints, extra=1000, fill=777), lens, dev)          # a larger Nmax; what lies behind an utterance is not read
    assert np.array_equal(frames, frames_w) and np.array_equal(as_f32, wide)
    for b, s in enumerate(ints):                                                       # each utterance alone
        alone, n = run_raw(mf, pad([s]), [lens[b]], dev)
        assert n[0] == frames[b] and np.array_equal(alone[0, :n[0]], as_f32[b, :n[0]]), b
    f2, n2 = mf([s.astype(np.int16) for s in ints])
    assert np.array_equal(f2.cpu().numpy(), as_f32[:, :98]) and np.array_equal(n2.cpu().numpy(), frames)
    f3, _ = mf(torch.from_numpy(pad(ints)), lens)
    assert torch.equal(f3, f2)


@pytest.mark.parametrize("kw", [dict(), dict(htk_compat=True), dict(htk_compat=True, use_energy=False, num_mel_bins=80, num_ceps=64)],
                         ids=["defaults", "htk", "htk_c0_64ceps"])
def test_fused_normalisation_is_the_float32_expression(dev, kw):
    mf = features.Mfcc(features.MfccConfig(dither=0.0, **kw), dev)
    C = mf.feat_dim
    rs = np.random.RandomState(5)
    mean = (3.0 * rs.standard_normal(C)).astype(np.float32)              # per column, after the HTK reordering
    scale = (0.2 + rs.random_sample(C)).astype(np.float32)
    lens = [s.shape[0] for s in SIGNALS[:5]]
    raw, frames = run_raw(mf, pad(SIGNALS[:5]), lens, dev)
    fused, frames_f = run_raw(mf, pad(SIGNALS[:5]), lens, dev, mean=torch.from_numpy(mean).to(dev), scale=torch.from_numpy(scale).to(dev))
    check_rows(fused, frames_f, lens, mf)
    assert np.array_equal(frames, frames_f)
    for b, n in enumerate(frames):
        want = ((raw[b, :n] - mean[None, :]) * scale[None, :]).astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(fused[b, :n], want), b
    f2, _ = mf(SIGNALS[:5], mean=mean, scale=scale)
    assert np.array_equal(f2.cpu().numpy(), fused[:, :98])


def test_dither(dev):
    mf = features.Mfcc(features.MfccConfig(dither=1.0), dev)
    sig = SIGNALS[1:5]
    a, n = mf(sig, seed=11)
    b, _ = mf(sig, seed=11)
    c, _ = mf(sig, seed=12)
    d, _ = mf(sig, seed=11, utt_offset=1)
    quiet, _ = features.Mfcc(features.MfccConfig(dither=0.0), dev)(sig)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d) and not torch.equal(a, quiet)
    for k in (2, 3):                                                    # utterance k of the batch, alone, behind utt_offset = k
        alone, m = mf([sig[k]], seed=11, utt_offset=k)
        assert int(m[0]) == int(n[k]) and torch.equal(alone[0, :int(m[0])], a[k, :int(n[k])]), k


def test_refusals_come_before_any_launch(dev):
    cases = ((dict(num_mel_bins=80, num_ceps=65), -3), (dict(frame_length=100.0), -3), (dict(num_ceps=0), -1), (dict(num_ceps=24), -1),
             (dict(cepstral_lifter=-1.0), -1))
    for kw, code in cases:
        with pytest.raises(RuntimeError, match="rc=%d" % code):
            features.Mfcc(features.MfccConfig(**kw), dev)
        opts = features.MfccConfig(**kw).c_opts()
        x = torch.zeros(1, 4000, device=dev)
        out = torch.full((1, 8, 130), SENTINEL, device=dev)
        n = torch.full((1,), -7777, dtype=torch.int32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert _lib.lib().ctcn_mfcc(p(x), 0, p(n), ctypes.byref(opts), p(x), None, None, p(out), p(n), 1, 4000, 8, 0.0, 0, 0, _lib.stream_ptr()) == code
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and int(n[0]) == -7777
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mfcc(torch.zeros(1, 400), [400], features.Mfcc(features.MfccConfig(), dev).plan)


def test_make_feat_end_to_end(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    rs = np.random.RandomState(77)
    lengths = [9000, 4801, 16000, 7777, 12345, 5600]
    waves, lines = [], []
    for i, n in enumerate(lengths):
        t = np.arange(n) / 16000.0
        x = 2000.0 * rs.standard_normal(n) * (0.3 + np.abs(np.sin(2 * np.pi * (1.0 + i) * t))) + 3000.0 * np.sin(2 * np.pi * (200.0 + 150.0 * i) * t)
        x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
        path = str(tmp_path / ("utt%d.wav" % i))
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(x.astype("<i2").tobytes())
        waves.append(x)
        lines.append("spk_utt%d %s\n" % (i, path))
    (tmp_path / "wav.scp").write_text("".join(lines))
    (tmp_path / "mfcc.conf").write_text("--use-energy=false   # only non-default option.\n--dither=0  # deterministic\n")
    out_dir = str(tmp_path / "feat")
    log = []
    common = ["--wav-scp", str(tmp_path / "wav.scp")]
    ark, scp = make_feat.main(common + ["--feat-type", "mfcc", "--conf", str(tmp_path / "mfcc.conf"), "--out-dir", out_dir, "--compute-cmvn"],
                              log=log.append)
    entries = [l.split() for l in open(scp)]
    assert [e[0] for e in entries] == ["spk_utt%d" % i for i in range(6)]
    mats = [read_kaldi_matrix(e[1]) for e in entries]
    mf = features.Mfcc(features.MfccConfig.from_kaldi_conf(str(tmp_path / "mfcc.conf")), dev)
    assert [m.shape for m in mats] == [(mf.num_frames(n), 13) for n in lengths]
    allf = np.concatenate(mats).astype(np.float64)
    print("make_feat mfcc: %d frames, max |mean| %.3g, max |var - 1| %.3g" % (allf.shape[0], np.abs(allf.mean(0)).max(), np.abs(allf.var(0) - 1).max()))
    assert np.abs(allf.mean(axis=0)).max() <= 1e-4 and np.abs(allf.var(axis=0) - 1.0).max() <= 1e-3
    # by hand, in the driver's order (by length): the statistics' float64 sums are taken in batch order
    order = sorted(range(6), key=lambda i: lengths[i])
    raw, frames = mf([waves[i] for i in order])
    cmvn = features.GlobalCMVN(13, dev).accumulate(raw, frames)
    stats_path = os.path.join(out_dir, "global_mfcc_cmvn.txt")
    assert sorted(os.listdir(out_dir)) == ["feats.ark", "feats.scp", "global_mfcc_cmvn.txt"]
    stats_file = features.GlobalCMVN.load_kaldi_text(stats_path)
    assert torch.equal(stats_file.stats, cmvn.stats.cpu()) and int(cmvn.stats[0, 13]) == allf.shape[0]
    mean, scale = cmvn.mean_scale()
    normed, _ = mf([waves[i] for i in order], mean=mean, scale=scale)
    for j, i in enumerate(order):
        assert np.array_equal(normed[j, :mats[i].shape[0]].cpu().numpy(), mats[i]), i
    # a second list normalised with the first one's statistics, in other batches (20 000 padded samples per launch): the same features
    make_feat.main(common + ["--feat-type", "mfcc", "--conf", str(tmp_path / "mfcc.conf"), "--out-dir", str(tmp_path / "feat2"),
                             "--cmvn-stats", stats_path, "--max-samples", "20000"], log=log.append)
    again = [read_kaldi_matrix(l.split()[1]) for l in open(str(tmp_path / "feat2" / "feats.scp"))]
    assert all(np.array_equal(x, y) for x, y in zip(again, mats))
    # without --feat-type the driver is the filterbank's: its statistics file name, 81 dimensions for the fbank conf
    (tmp_path / "fbank.conf").write_text("--window-type=hamming\n--num-mel-bins=80\n--use-energy\n--dither=0\n")
    _, scp3 = make_feat.main(common + ["--conf", str(tmp_path / "fbank.conf"), "--out-dir", str(tmp_path / "feat3"), "--compute-cmvn"], log=log.append)
    assert sorted(os.listdir(str(tmp_path / "feat3"))) == ["feats.ark", "feats.scp", "global_fbank_cmvn.txt"]
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf")), dev)
    m3 = [read_kaldi_matrix(l.split()[1]) for l in open(scp3)]
    assert [m.shape for m in m3] == [(fb.num_frames(n), 81) for n in lengths]
    fstats = features.GlobalCMVN(81, dev).accumulate(*fb([waves[i] for i in order]))
    fmean, fscale = fstats.mean_scale()
    fnorm, _ = fb([waves[i] for i in order], mean=fmean, scale=fscale)
    for j, i in enumerate(order):
        assert np.array_equal(fnorm[j, :m3[i].shape[0]].cpu().numpy(), m3[i]), i
