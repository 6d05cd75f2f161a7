"""Host-side checks of the filterbank front-end (no GPU): the frame-count query, the plan builder against the numpy restatement of Kaldi's
window and mel bank (tests/fbank_ref.py), the Kaldi config reader, the wave readers, the CMVN text file and the driver's argument parser.

Bounds.  Window: both sides evaluate the same double expression and round once to float32; cos / pow of two maths libraries may differ in
the last place of the double, which can move the rounding by one float32 ulp.  Weights: values in [0, 1] computed in double on both
sides and rounded once (6e-8); 1e-6 leaves room for the last-place differences of log."""
import ctypes
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fbank_ref as R  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_of(**kw):
    return ops.FbankPlan(features.FbankConfig(**kw).c_opts())


@pytest.mark.parametrize("snip", [True, False])
def test_frame_count_agrees_with_kaldis_two_formulas(snip):
    L, shift = 400, 160
    for n in (0, 1, 399, 400, 401, 559, 560, 561, 16037):
        want = (0 if n < L else 1 + (n - L) // shift) if snip else (n + shift // 2) // shift
        assert ops.fbank_frames(n, L, shift, snip) == want == R.num_frames(n, L, shift, snip), (n, snip)
    assert ops.fbank_frames(16037, 400, 160, True) == 98 and ops.fbank_frames(16037, 400, 160, False) == 100
    fn = _lib.lib().ctcn_fbank_frames
    assert fn(100, 0, 160, 1) < 0 and fn(100, 400, 0, 1) < 0 and fn(-1, 400, 160, 1) < 0
    with pytest.raises(ValueError):
        ops.fbank_frames(100, 0, 160)


@pytest.mark.parametrize("rate", [8000.0, 16000.0])
@pytest.mark.parametrize("bins", [23, 40, 80])
def test_plan_against_the_restatement(rate, bins):
    for wt in features.WINDOW_TYPES:
        kw = dict(sample_frequency=rate, num_mel_bins=bins, window_type=wt, htk_compat=(wt == "hanning"))
        plan, o = plan_of(**kw), R.options(**kw)
        L, shift, npad = R.geometry(o)
        assert (plan.frame_length, plan.frame_shift, plan.padded_length) == (L, shift, npad) == ((200, 80, 256) if rate == 8000.0 else (400, 160, 512))
        f32, i32 = plan.host.view(np.float32), plan.host.view(np.int32)
        assert plan.host.size == 6 * npad + 384
        # window: within 1 float32 ulp, zero from the frame length on
        want = R.window(o).astype(np.float32)
        got = f32[:npad]
        ulps = np.abs(got[:L].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert int(ulps.max()) <= 1, (wt, int(ulps.max()))
        assert not got[L:].any()
        # twiddles: exp(-2 pi i k / npad)
        k = np.arange(npad)
        tw = plan.host[npad:5 * npad].view(np.float64).reshape(npad, 2)
        assert np.abs(tw[:, 0] - np.cos(2 * np.pi * k / npad)).max() <= 3e-16 and np.abs(tw[:, 1] + np.sin(2 * np.pi * k / npad)).max() <= 3e-16
        # mel bank: identical ranges, weights within 1e-6, every bin in at most two filters, no empty filter
        first, count, woff = (i32[5 * npad + 128 * j:5 * npad + 128 * j + bins] for j in range(3))
        wts = f32[5 * npad + 384:]
        bank = R.mel_bank(o)
        feeds = np.zeros(npad // 2, dtype=int)
        for b, (ref_first, ref_w) in enumerate(bank):
            assert (int(first[b]), int(count[b])) == (ref_first, ref_w.size) and count[b] >= 1, (b, first[b], count[b])
            assert np.abs(wts[woff[b]:woff[b] + count[b]] - ref_w).max() <= 1e-6
            feeds[first[b]:first[b] + count[b]] += 1
        assert feeds.max() <= 2 and int(woff[bins - 1] + count[bins - 1]) <= npad
        assert np.array_equal(woff, np.concatenate([[0], np.cumsum(count)[:-1]]))


def test_plan_refuses_what_the_kernel_does_not_take():
    for kw, code in ((dict(frame_length=100.0), -3), (dict(num_mel_bins=129), -3), (dict(round_to_power_of_two=False), -3),
                     (dict(frame_length=5.0), -3), (dict(num_mel_bins=2), -1), (dict(sample_frequency=8000.0, num_mel_bins=128), -1),
                     (dict(low_freq=9000.0), -1)):
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            plan_of(**kw)
        if code == -3:
            assert _lib.lib().ctcn_fbank_plan_bytes(ctypes.byref(features.FbankConfig(**kw).c_opts())) == 0
    assert plan_of(frame_length=50.0).padded_length == 1024
    o = features.FbankConfig().c_opts()
    assert _lib.lib().ctcn_fbank_plan(ctypes.byref(o), None, 0) == -1 and _lib.lib().ctcn_fbank_plan(None, None, 0) == -1


def test_ops_raise_for_cpu_tensors():
    plan = plan_of()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fbank(torch.zeros(1, 400), [400], plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cmvn_accumulate(torch.zeros(1, 2, 23), torch.tensor([2], dtype=torch.int32), torch.zeros(2, 24, dtype=torch.float64))


def test_kaldi_conf_reader(tmp_path):
    conf = tmp_path / "fbank.conf"
    conf.write_text("# the reference's conf/fbank.conf\n--window-type=hamming\n--num-mel-bins=80\n\n--use-energy   # a bare flag\n")
    c = features.FbankConfig.from_kaldi_conf(str(conf))
    assert (c.window_type, c.num_mel_bins, c.use_energy, c.feat_dim) == ("hamming", 80, True, 81)
    d = features.FbankConfig.DEFAULTS
    assert all(getattr(c, k) == v for k, v in d.items() if k not in ("window_type", "num_mel_bins", "use_energy"))
    assert d == R.DEFAULTS and d["dither"] == 1.0 and d["window_type"] == "povey" and d["num_mel_bins"] == 23
    conf.write_text("--dither=0\n--snip-edges=false\n--sample-frequency=8000\n--energy-floor=1.5\n")
    c = features.FbankConfig.from_kaldi_conf(str(conf))
    assert (c.dither, c.snip_edges, c.sample_frequency, c.energy_floor) == (0.0, False, 8000.0, 1.5)
    conf.write_text("--num-mel-bins=80\n--vtln-warp=1.1\n")
    with pytest.raises(ValueError, match="vtln-warp"):
        features.FbankConfig.from_kaldi_conf(str(conf))
    conf.write_text("num-mel-bins=80\n")
    with pytest.raises(ValueError):
        features.FbankConfig.from_kaldi_conf(str(conf))
    with pytest.raises(ValueError):
        features.FbankConfig(window_type="kaiser")


def sphere_bytes(samples, order, rate=16000, coding="pcm", nbytes=2):
    head = "NIST_1A\n   1024\nchannel_count -i 1\nsample_count -i %d\nsample_rate -i %d\nsample_n_bytes -i %d\n" % (len(samples), rate, nbytes)
    head += "sample_byte_format -s2 %s\nsample_coding -s%d %s\nsample_sig_bits -i 16\nend_head\n" % (order, len(coding), coding)
    return head.encode().ljust(1024) + np.asarray(samples).astype("<i2" if order == "01" else ">i2").tobytes()


def test_read_wave(tmp_path):
    x = (np.random.RandomState(0).randint(-32768, 32768, size=1234)).astype(np.int16)
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(x.astype("<i2").tobytes())
    got, rate = features.read_wave(p)
    assert rate == 8000 and got.dtype == np.int16 and np.array_equal(got, x)
    for order in ("01", "10"):
        p = str(tmp_path / ("s%s.wav" % order))
        open(p, "wb").write(sphere_bytes(x, order))
        got, rate = features.read_wave(p)
        assert rate == 16000 and got.dtype == np.int16 and np.array_equal(got, x), order
    p = str(tmp_path / "ulaw.wav")
    open(p, "wb").write(sphere_bytes(x, "1", coding="ulaw", nbytes=1))
    with pytest.raises(NotImplementedError, match="ulaw"):
        features.read_wave(p)
    open(p, "wb").write(sphere_bytes(x, "01", coding="pcm,embedded-shorten-v2.00"))
    with pytest.raises(NotImplementedError, match="shorten"):
        features.read_wave(p)
    # RIFF with a mu-law format tag (7), and stereo PCM
    fmt = struct.pack("<HHIIHH", 7, 1, 8000, 8000, 1, 8)
    open(p, "wb").write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + 4) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", 4) + b"\0" * 4)
    with pytest.raises(NotImplementedError, match="format tag 7"):
        features.read_wave(p)
    with wave.open(p, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(b"\0" * 8)
    with pytest.raises(NotImplementedError, match="2 channel"):
        features.read_wave(p)
    open(p, "wb").write(b"OggS" + b"\0" * 60)
    with pytest.raises(NotImplementedError):
        features.read_wave(p)


def test_global_cmvn_text_round_trip_and_mean_scale(tmp_path):
    c = features.GlobalCMVN(3)
    # 4 frames: column 0 = (1, 1, 3, 3): mean 2, var 1; column 1 constant 5: var floors at 1e-20; column 2 = (0, 0, 0, 8): mean 2, var 12
    c.stats.copy_(torch.tensor([[8.0, 20.0, 8.0, 4.0], [20.0, 100.0, 64.0, 0.0]], dtype=torch.float64))
    mean, scale = c.mean_scale()
    assert mean.dtype == scale.dtype == np.float32
    assert np.array_equal(mean, np.float32([2, 5, 2]))
    assert np.array_equal(scale, np.array([1.0, 1e10, 1.0 / np.sqrt(12.0)]).astype(np.float32))
    rm, rs = R.mean_scale(c.stats.numpy())
    assert np.array_equal(mean, rm) and np.array_equal(scale, rs)
    c.stats[0, 0] = 1.0 / 3.0                                           # a value that needs all its digits
    p = str(tmp_path / "global_fbank_cmvn.txt")
    c.save_kaldi_text(p)
    text = open(p).read()
    assert text.startswith(" [\n  ") and text.endswith(" ]\n") and text.count("\n") == 3     # Kaldi's text matrix layout
    back = features.GlobalCMVN.load_kaldi_text(p)
    assert back.feat_dim == 3 and torch.equal(back.stats, c.stats)
    # what compute-cmvn-stats writes into an archive: the same matrix behind a key, six significant digits
    open(p, "w").write("global  [\n  8 20 8 4 \n  20 100 64 0 ]\n")
    back = features.GlobalCMVN.load_kaldi_text(p)
    assert back.stats.tolist() == [[8.0, 20.0, 8.0, 4.0], [20.0, 100.0, 64.0, 0.0]]
    with pytest.raises(ValueError):
        features.GlobalCMVN(3).mean_scale()
    open(p, "w").write(" [\n 1 2 3 ]\n")
    with pytest.raises(ValueError):
        features.GlobalCMVN.load_kaldi_text(p)


def test_restatement_float32_follows_float64():
    """The yardstick's two precisions on one second of noise, and one frame of the float64 one by hand.  The float32 chain is held to the
    float64 one only grossly here (1e-2: a slip in either moves values by tenths; its true distance, which the lowest filters set -- DC
    removal and pre-emphasis leave them 1e-5 of the spectrum's power, so float32 FFT noise weighs 1e-4 .. 1e-3 there -- is what the GPU
    test measures as e32), and typically (median) to float32 rounding of values around 20."""
    x = np.round(3000.0 * np.random.RandomState(1).standard_normal(16037))
    o = R.options(window_type="hamming", num_mel_bins=80, use_energy=True, dither=0.0)
    a, b = R.fbank(x, o, np.float64), R.fbank(x, o, np.float32)
    assert a.shape == b.shape == (98, 81) and b.dtype == np.float32 and a.min() > 5.0
    assert np.abs(a - b).max() < 1e-2 and np.median(np.abs(a - b)) < 4e-6
    # a frame by hand: the DFT sum of the windowed, pre-emphasised, mean-free first frame
    f = x[:400] - x[:400].mean()
    e0 = np.log((f * f).sum())
    f = (f - np.float64(np.float32(0.97)) * np.concatenate([f[:1], f[:-1]])) * R.window(o)
    k, n = np.arange(256)[:, None], np.arange(400)[None, :]
    power = np.abs((f[None, :] * np.exp(-2j * np.pi * k * n / 512)).sum(axis=1)) ** 2
    first, w = R.mel_bank(o)[37]
    assert abs(a[0, 0] - e0) < 1e-12 and abs(a[0, 38] - np.log((power[first:first + w.size] * w).sum())) < 1e-9


def test_make_feat_help_parses():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "ctc_pytorch_amd", "steps", "make_feat.py"), "--help"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "--compute-cmvn" in p.stdout and "--wav-scp" in p.stdout, p.stderr[-400:]
    from ctc_pytorch_amd.steps import make_feat
    assert make_feat.length_batches([5, 1, 9, 9, 2], 18) == [[1, 4, 0], [2, 3]]
    assert make_feat.length_batches([100, 3], 10) == [[1], [0]]
