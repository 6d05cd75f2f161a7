"""The filterbank front-end on the HIP kernels (ctcn_fbank through its C entry point, ops.fbank, utils/features.Fbank; ctcn_cmvn_accumulate
through ops.cmvn_accumulate and GlobalCMVN; steps/make_feat.py) against the numpy restatement of Kaldi's algorithm in tests/fbank_ref.py.

Parity bound.  e32 = the largest absolute difference between the float32 and the float64 restatement on the same batch and configuration
(float32 with scipy's single-precision rfft and BLAS dot products); the kernel's largest difference to the float64 restatement must stay
within 4 * e32, and within 1e-5 where 4 * e32 is smaller: the kernel does the same 24-bit arithmetic with its butterflies and its filter
sums in another order.  e32 comes from the two restatements alone.  With use_log_fbank=false both differences are taken relative to the
float64 value.  Every test prints its figures before it asserts; the measured ones are in DESIGN.md section 7h."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fbank_ref as R  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402
from ctc_pytorch_amd.utils.data_loader import read_kaldi_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
LOG_EPS = float(np.log(np.float32(np.finfo(np.float32).eps).astype(np.float64)))
LENS = [0, 399, 400, 1360, 16037]           # no frame | one sample short of a frame | the frame that ends on the last sample | 7 frames | 98
SHIPPED = dict(window_type="hamming", num_mel_bins=80, use_energy=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def make_signals():
    """The six utterances of the parity batches as float32 on Kaldi's scale, from one seeded generator."""
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
_REF = {}


def reference(key, batch_index, **kw):
    """[(float64 features, float32 features)] per utterance of a batch; computed once per configuration and shared."""
    k = (key, batch_index)
    if k not in _REF:
        o = R.options(dither=0.0, **kw)
        _REF[k] = [(R.fbank(s, o, np.float64), R.fbank(s, o, np.float32)) for s in BATCHES[batch_index]]
    return _REF[k]


def pad(signals, dtype=np.float32, extra=0, fill=0):
    out = np.full((len(signals), max(max(s.shape[0] for s in signals), 1) + extra), fill, dtype=dtype)
    for b, s in enumerate(signals):
        out[b, :s.shape[0]] = s
    return out


def run_raw(fb, batch, lens, dev, extra_rows=3, mean=None, scale=None, dither=0.0, seed=0, utt_offset=0):
    """ctcn_fbank called directly, outputs pre-filled with a sentinel, `extra_rows` rows more than any utterance needs."""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    w = torch.from_numpy(batch).to(dev)
    B, Nmax = batch.shape
    Tmax = max(fb.num_frames(n) for n in lens) + extra_rows
    feats = torch.full((B, Tmax, fb.feat_dim), 12345.0, dtype=torch.float32, device=dev)
    frames = torch.full((B,), -7777, dtype=torch.int32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ctcn_fbank(p(w), int(batch.dtype == np.int16), p(lens_d), ctypes.byref(fb.plan.opts), p(fb.plan.on(dev)), p(mean), p(scale),
                                     p(feats), p(frames), B, Nmax, Tmax, float(dither), seed, utt_offset, _lib.stream_ptr()), "fbank")
    return feats.cpu().numpy(), frames.cpu().numpy()


def check_rows(feats, frames, lens, fb):
    """frames exact, every element written, every row at or beyond frames[b] exactly zero."""
    assert frames.tolist() == [fb.num_frames(n) for n in lens], (frames, lens)
    assert not (feats == 12345.0).any()
    for b, n in enumerate(frames):
        assert not feats[b, n:].any(), (b, n)


PARITY = {
    "kaldi_defaults": dict(),
    "shipped": SHIPPED,
    "8khz_23bins": dict(sample_frequency=8000.0, num_mel_bins=23, window_type="hamming"),
    "40bins": dict(num_mel_bins=40, window_type="hamming"),
    "energy_after_window": dict(SHIPPED, raw_energy=False),
    "htk_compat": dict(SHIPPED, htk_compat=True),
    "no_preemphasis": dict(SHIPPED, preemphasis_coefficient=0.0),
    "keep_dc_offset": dict(SHIPPED, remove_dc_offset=False),
    "hamming": dict(num_mel_bins=80, window_type="hamming"),
    "hanning": dict(num_mel_bins=80, window_type="hanning"),
    "povey": dict(num_mel_bins=80, window_type="povey"),
    "rectangular": dict(num_mel_bins=80, window_type="rectangular"),
    "blackman": dict(num_mel_bins=80, window_type="blackman", blackman_coeff=0.40),
    "magnitude": dict(SHIPPED, use_power=False),
    "linear": dict(num_mel_bins=80, window_type="hamming", use_log_fbank=False),
    "reflected_edges": dict(SHIPPED, snip_edges=False),
    "energy_floor": dict(SHIPPED, energy_floor=3.6e9),                   # 400 samples of sigma 3000: about half the frames lie below
    "50ms_1024": dict(SHIPPED, frame_length=50.0),
}


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_with_the_restatement(dev, name):
    kw = PARITY[name]
    fb = features.Fbank(features.FbankConfig(dither=0.0, **kw), dev)
    relative = not kw.get("use_log_fbank", True)
    worst_k = worst_32 = 0.0
    lowest = np.inf
    for bi, signals in enumerate(BATCHES):
        lens = [s.shape[0] for s in signals]
        ref = reference(name, bi, **kw)
        feats, frames = run_raw(fb, pad(signals), lens, dev)
        check_rows(feats, frames, lens, fb)
        e32 = ek = 0.0
        for b, (r64, r32) in enumerate(ref):
            assert r64.shape == (frames[b], fb.feat_dim)
            if not r64.size:
                continue
            den = np.abs(r64) if relative else 1.0
            e32 = max(e32, float((np.abs(r32.astype(np.float64) - r64) / den).max()))
            ek = max(ek, float((np.abs(feats[b, :frames[b]].astype(np.float64) - r64) / den).max()))
            lowest = min(lowest, float(r64.min()))
        print("%s batch %d: e32 %.3g, kernel %.3g, bound %.3g, lowest value %.4g" % (name, bi, e32, ek, max(4 * e32, 1e-5), lowest))
        assert ek <= max(4.0 * e32, 1e-5), (name, bi, ek, e32)
        worst_k, worst_32 = max(worst_k, ek), max(worst_32, e32)
        if bi == 0:                                                     # the Python surface gives the same bits, without the spare rows
            f2, n2 = fb(signals)
            assert np.array_equal(n2.cpu().numpy(), frames) and np.array_equal(f2.cpu().numpy(), feats[:, :f2.shape[1]])
    if name == "energy_floor":
        r64 = reference(name, 0, **kw)[4][0]
        floor = np.log(np.float64(np.float32(3.6e9)))
        assert (r64[:, 0] == floor).any() and (r64[:, 0] > floor).any()    # the floor bites on some frames only


def test_silence_sits_on_the_floor(dev):
    fb = features.Fbank(features.FbankConfig(dither=0.0, **SHIPPED), dev)
    feats, frames = fb([np.zeros(4000, dtype=np.float32), np.zeros(400, dtype=np.int16).astype(np.float32)])
    feats, frames = feats.cpu().numpy(), frames.cpu().numpy()
    assert frames.tolist() == [23, 1]
    real = np.concatenate([feats[0, :23], feats[1, :1]])
    print("silence: max |x - log(FLT_EPSILON)| = %.3g" % np.abs(real - LOG_EPS).max())
    assert np.abs(real.astype(np.float64) - LOG_EPS).max() <= 1e-6
    assert not feats[1, 1:].any()


def test_batch_invariance_and_input_types(dev):
    fb = features.Fbank(features.FbankConfig(dither=0.0, **SHIPPED), dev)
    ints = [np.clip(np.round(s), -32768, 32767) for s in SIGNALS[:5]]
    lens = [s.shape[0] for s in ints]
    as_f32, frames = run_raw(fb, pad(ints), lens, dev)
    check_rows(as_f32, frames, lens, fb)
    assert frames.tolist() == [0, 0, 1, 7, 98]
    as_i16, frames_i = run_raw(fb, pad(ints, np.int16), lens, dev)
    assert np.array_equal(frames, frames_i) and np.array_equal(as_f32, as_i16)
    wide, frames_w = run_raw(fb, pad(ints, extra=1000, fill=777), lens, dev)          # a larger Nmax; what lies behind an utterance is not read
    assert np.array_equal(frames, frames_w) and np.array_equal(as_f32, wide)
    for b, s in enumerate(ints):                                                       # each utterance alone
        for dtype in (np.float32, np.int16):
            alone, n = run_raw(fb, pad([s], dtype), [lens[b]], dev)
            assert n[0] == frames[b] and np.array_equal(alone[0, :n[0]], as_f32[b, :n[0]]), (b, dtype)
    f2, n2 = fb([s.astype(np.int16) for s in ints])
    assert np.array_equal(f2.cpu().numpy(), as_f32[:, :98]) and np.array_equal(n2.cpu().numpy(), frames)
    f3, _ = fb(torch.from_numpy(pad(ints)), lens)
    assert torch.equal(f3, f2)


def test_fused_normalisation_is_the_float32_expression(dev):
    fb = features.Fbank(features.FbankConfig(dither=0.0, **SHIPPED), dev)
    rs = np.random.RandomState(5)
    mean = (15.0 + 5.0 * rs.standard_normal(81)).astype(np.float32)
    scale = (0.2 + rs.random_sample(81)).astype(np.float32)
    lens = [s.shape[0] for s in SIGNALS[:5]]
    raw, frames = run_raw(fb, pad(SIGNALS[:5]), lens, dev)
    fused, frames_f = run_raw(fb, pad(SIGNALS[:5]), lens, dev, mean=torch.from_numpy(mean).to(dev), scale=torch.from_numpy(scale).to(dev))
    check_rows(fused, frames_f, lens, fb)
    assert np.array_equal(frames, frames_f)
    for b, n in enumerate(frames):
        want = ((raw[b, :n] - mean[None, :]) * scale[None, :]).astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(fused[b, :n], want), b
    f2, _ = fb(SIGNALS[:5], mean=mean, scale=scale)
    assert np.array_equal(f2.cpu().numpy(), fused[:, :98])


def test_cmvn_statistics(dev):
    rs = np.random.RandomState(9)
    B, Tmax, F = 5, 130, 81
    a = (10.0 + 4.0 * rs.standard_normal((B, Tmax, F))).astype(np.float32)
    fa = [130, 64, 65, 0, 1]                                            # the chunk of 64 rows: full, exactly one, one row more, none, one row
    fb = features.Fbank(features.FbankConfig(dither=0.0, **SHIPPED), dev)
    feats_b, frames_b = fb(SIGNALS[:5])
    b_host, fb_host = feats_b.cpu().numpy(), frames_b.cpu().numpy().tolist()

    def run():
        c = features.GlobalCMVN(F, dev)
        x = torch.from_numpy(a).to(dev)
        for i, n in enumerate(fa):
            x[i, n:] = float("nan")                                     # padded rows are never read
        c.accumulate(x, torch.tensor(fa, dtype=torch.int32, device=dev))
        y = feats_b.clone()
        for i, n in enumerate(fb_host):
            y[i, n:] = float("nan")
        c.accumulate(y, frames_b)
        return c

    c1, c2 = run(), run()
    got = c1.stats.cpu().numpy()
    assert np.array_equal(got, c2.stats.cpu().numpy())                  # bit for bit, run to run
    want = R.cmvn_stats([a[i, :n] for i, n in enumerate(fa)] + [b_host[i, :n] for i, n in enumerate(fb_host)])
    assert got[0, F] == want[0, F] == sum(fa) + sum(fb_host) and got[1, F] == 0.0
    rel = np.abs(got[:, :F] - want[:, :F]) / np.abs(want[:, :F])
    print("cmvn: max relative difference to float64 numpy %.3g over %d frames" % (rel.max(), int(got[0, F])))
    assert rel.max() <= 1e-10
    m, s = c1.mean_scale()
    rm, rsd = R.mean_scale(got)
    assert np.array_equal(m, rm) and np.array_equal(s, rsd)


def test_dither(dev):
    cfg = features.FbankConfig(dither=1.0, **SHIPPED)
    fb = features.Fbank(cfg, dev)
    sig = SIGNALS[1:5]
    a, n = fb(sig, seed=11)
    b, _ = fb(sig, seed=11)
    c, _ = fb(sig, seed=12)
    quiet, _ = features.Fbank(features.FbankConfig(dither=0.0, **SHIPPED), dev)(sig)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, quiet)
    for k in (2, 3):                                                    # utterance k of the batch, alone, behind utt_offset = k
        alone, m = fb([sig[k]], seed=11, utt_offset=k)
        assert int(m[0]) == int(n[k]) and torch.equal(alone[0, :int(m[0])], a[k, :int(n[k])]), k
        shifted, _ = fb([sig[k]], seed=11, utt_offset=k + 1)
        assert not torch.equal(shifted, alone)
    # the noise itself: zero signal, nothing between the samples and the energy but the sum of squares
    sigma = 2.5
    plain = features.Fbank(features.FbankConfig(dither=sigma, window_type="rectangular", preemphasis_coefficient=0.0, remove_dc_offset=False,
                                                use_energy=True, raw_energy=True, num_mel_bins=23), dev)
    feats, frames = plain([np.zeros(400 + 160 * 99, dtype=np.float32)] * 5, seed=3)
    assert frames.tolist() == [100] * 5
    var = np.exp(feats[:, :, 0].double().cpu().numpy()) / 400.0          # per frame: the mean square of 400 samples of noise
    print("dither: mean square / sigma^2 = %.4f over %d frames" % (var.mean() / sigma ** 2, var.size))
    assert abs(var.mean() / sigma ** 2 - 1.0) <= 0.05
    assert not np.array_equal(var[0], var[1])                           # utterances draw their own noise


def test_refusals_come_before_any_launch(dev):
    for kw in (dict(frame_length=100.0), dict(num_mel_bins=129), dict(round_to_power_of_two=False)):
        with pytest.raises(RuntimeError, match="rc=-3"):
            features.Fbank(features.FbankConfig(**kw), dev)
        opts = features.FbankConfig(**kw).c_opts()
        x = torch.zeros(1, 4000, device=dev)
        out = torch.full((1, 8, 130), 12345.0, device=dev)
        n = torch.full((1,), -7777, dtype=torch.int32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert _lib.lib().ctcn_fbank(p(x), 0, p(n), ctypes.byref(opts), p(x), None, None, p(out), p(n), 1, 4000, 8, 0.0, 0, 0, _lib.stream_ptr()) == -3
        torch.cuda.synchronize()
        assert bool((out == 12345.0).all()) and int(n[0]) == -7777
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fbank(torch.zeros(1, 400), [400], features.Fbank(features.FbankConfig(), dev).plan)


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
    (tmp_path / "fbank.conf").write_text("--window-type=hamming\n--num-mel-bins=80\n--use-energy\n--dither=0  # deterministic\n")
    out_dir = str(tmp_path / "feat")
    log = []
    ark, scp = make_feat.main(["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp"), "--out-dir", out_dir, "--compute-cmvn"],
                              log=log.append)
    entries = [l.split() for l in open(scp)]
    assert [e[0] for e in entries] == ["spk_utt%d" % i for i in range(6)]
    mats = [read_kaldi_matrix(e[1]) for e in entries]
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf")), dev)
    assert [m.shape for m in mats] == [(fb.num_frames(n), 81) for n in lengths]
    allf = np.concatenate(mats).astype(np.float64)
    print("make_feat: %d frames, max |mean| %.3g, max |var - 1| %.3g" % (allf.shape[0], np.abs(allf.mean(0)).max(), np.abs(allf.var(0) - 1).max()))
    assert np.abs(allf.mean(axis=0)).max() <= 1e-4 and np.abs(allf.var(axis=0) - 1.0).max() <= 1e-3
    # by hand, in the driver's order (by length): the statistics' float64 sums are taken in batch order
    order = sorted(range(6), key=lambda i: lengths[i])
    raw, frames = fb([waves[i] for i in order])
    cmvn = features.GlobalCMVN(81, dev).accumulate(raw, frames)
    stats_file = features.GlobalCMVN.load_kaldi_text(os.path.join(out_dir, "global_fbank_cmvn.txt"))
    assert torch.equal(stats_file.stats, cmvn.stats.cpu()) and int(cmvn.stats[0, 81]) == allf.shape[0]
    mean, scale = cmvn.mean_scale()
    normed, _ = fb([waves[i] for i in order], mean=mean, scale=scale)
    for j, i in enumerate(order):
        assert np.array_equal(normed[j, :mats[i].shape[0]].cpu().numpy(), mats[i]), i
    # a second list normalised with the first one's statistics
    make_feat.main(["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp"), "--out-dir", str(tmp_path / "feat2"),
                    "--cmvn-stats", os.path.join(out_dir, "global_fbank_cmvn.txt"), "--max-samples", "20000"], log=log.append)
    again = [read_kaldi_matrix(l.split()[1]) for l in open(str(tmp_path / "feat2" / "feats.scp"))]
    assert all(np.array_equal(x, y) for x, y in zip(again, mats))       # other batches (20 000 padded samples per launch), the same features
