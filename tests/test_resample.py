"""The resampler on the HIP kernel (ctcn_resample) through its C entry point, ops, utils/features (Resampler, SpeedPerturb) and
steps/make_feat.py (--speed-perturb, --text, allow_downsample / allow_upsample), against the numpy restatement of tests/resample_ref.py run on
the plan's own weights.  The demand is bit-identity: the kernel's sum is the ascending float64 sum of exact products, one number on any
machine (include/ctcn.h).  Signal lengths: test_resample_host.signal_lengths."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402
from test_resample_host import plan_of, signal_lengths  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402
from ctc_pytorch_amd.utils.data_loader import read_kaldi_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
PAIRS = RR.PAIRS
SENTINEL = -54321.0
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case(pair):
    """(plan, lengths, padded int16 batch, the restatement's output of every utterance), computed once per pair."""
    if pair not in _CASES:
        plan = plan_of(pair)
        lens = signal_lengths(pair, plan)
        rs = np.random.RandomState(pair[0] % 997 + 11)
        batch = np.zeros((len(lens), max(lens)), dtype=np.int16)
        want = []
        for b, n in enumerate(lens):
            batch[b, :n] = rs.randint(-32768, 32768, size=n)
            want.append(RR.resample(batch[b, :n], pair[0], pair[1], plan.first, plan.ntaps, plan.weights))
        _CASES[pair] = (plan, lens, batch, want)
    return _CASES[pair]


def run_raw(plan, batch, lens, dev, spare=5):
    """ctcn_resample called directly: the output pre-filled with a sentinel, `spare` columns more than any utterance needs."""
    w = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
    B, Nmax = batch.shape
    Mmax = max(RR.num_samples(n, plan.orig_freq, plan.new_freq) for n in lens) + spare
    out = torch.full((B, Mmax), SENTINEL, dtype=torch.float32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ctcn_resample(p(w), int(batch.dtype == np.int16), p(lens_d), ctypes.byref(plan.opts), p(plan.on(dev)), p(out), B, Nmax, Mmax,
                                        _lib.stream_ptr()), "resample")
    return out.cpu().numpy()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda q: "%d_%d" % q)
def test_kernel_is_the_restatement_bit_for_bit(pair, dev):
    plan, lens, batch, want = case(pair)
    out = run_raw(plan, batch, lens, dev)
    assert not np.any(out == SENTINEL), "elements left unwritten"
    for b, n in enumerate(lens):
        m = -((-n * pair[1]) // pair[0])
        assert want[b].shape[0] == m == ops.resample_samples(n, *pair)
        assert np.all(bits(out[b, m:]) == 0), (pair, n)                  # zeros (+0.0) from the utterance's length on
        assert np.array_equal(bits(out[b, :m]), bits(want[b])), (pair, n, int((bits(out[b, :m]) != bits(want[b])).sum()))


@pytest.mark.parametrize("pair", PAIRS, ids=lambda q: "%d_%d" % q)
def test_input_type_padding_batching_and_repetition_leave_the_bits(pair, dev):
    plan, lens, batch, _ = case(pair)
    base = run_raw(plan, batch, lens, dev)
    assert np.array_equal(bits(run_raw(plan, batch, lens, dev)), bits(base)), "two runs differ"
    as_float = batch.astype(np.float32)
    assert np.array_equal(bits(run_raw(plan, as_float, lens, dev)), bits(base)), "float32 input differs from int16"
    wide = np.full((batch.shape[0], batch.shape[1] + 41), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        wide[b, :n] = as_float[b, :n]
    assert np.array_equal(bits(run_raw(plan, wide, lens, dev)), bits(base)), "NaN behind the utterances reached the sums"
    for b, n in enumerate(lens):
        alone = run_raw(plan, batch[b:b + 1, :max(n, 1)], [n], dev, spare=2)
        m = RR.num_samples(n, *pair)
        assert np.array_equal(bits(alone[0, :m]), bits(base[b, :m])) and np.all(bits(alone[0, m:]) == 0), (pair, n)
    # a length beyond the row is clamped to it; a negative one is empty
    odd = run_raw(plan, batch[:2, :100], [250, -3], dev)
    assert np.array_equal(bits(odd[0]), bits(run_raw(plan, batch[:1, :100], [100], dev, spare=odd.shape[1] - RR.num_samples(100, *pair))[0]))
    assert np.all(bits(odd[1]) == 0)


def test_ops_resampler_and_speed_perturb(dev):
    pair = (14400, 16000)
    plan, lens, batch, want = case(pair)
    out, out_lens = ops.resample(torch.from_numpy(batch).to(dev), lens, plan)
    assert out_lens == [w.shape[0] for w in want] and tuple(out.shape) == (len(lens), max(out_lens)) and out.dtype == torch.float32
    host = out.cpu().numpy()
    for b, w in enumerate(want):
        assert np.array_equal(bits(host[b, :w.shape[0]]), bits(w)) and np.all(bits(host[b, w.shape[0]:]) == 0)
    out2, lens2 = ops.resample(torch.from_numpy(batch).to(dev), torch.tensor(lens), plan)          # lengths as a tensor
    assert lens2 == out_lens and torch.equal(out2, out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample(torch.from_numpy(batch), lens, plan)
    with pytest.raises(TypeError):
        ops.resample(torch.from_numpy(batch).to(dev), lens, features.Fbank(features.FbankConfig(), dev).plan)
    with pytest.raises(TypeError):
        ops.resample(torch.from_numpy(batch).to(dev).double(), lens, plan)
    with pytest.raises(ValueError):
        ops.resample(torch.from_numpy(batch).to(dev), lens[:-1], plan)
    # Resampler: a list of waveforms, or a padded batch with lengths -- what the raw call gives
    rs = features.Resampler(14400, 16000, dev)
    waves = [batch[b, :n] for b, n in enumerate(lens) if n > 0]
    kept = [b for b, n in enumerate(lens) if n > 0]
    got, got_lens = rs(waves)
    assert got_lens == [out_lens[b] for b in kept] and got.device.type == "cuda" and got.dtype == torch.float32
    assert all(np.array_equal(bits(got[j, :got_lens[j]].cpu().numpy()), bits(want[b])) for j, b in enumerate(kept))
    got, got_lens = rs(batch, lens)
    assert got_lens == out_lens and torch.equal(got, out)
    assert rs.num_samples(14400) == 16000
    # equal rates: the same samples come back
    same, same_lens = features.Resampler(16000, 16000, dev)(batch, lens)
    assert same_lens == lens and same.device.type == "cuda" and np.array_equal(same.cpu().numpy(), batch)
    # SpeedPerturb: one Resampler per factor; 0.9 at 16 kHz is 14400 -> 16000, 1.1 is 17600 -> 16000, 1.0 the identity
    sp = features.SpeedPerturb(16000, device=dev)
    assert sp.factors == (0.9, 1.0, 1.1) and sp.resamplers[0.9].plan.orig_freq == 14400 and sp.resamplers[1.1].plan.orig_freq == 17600
    slow, slow_lens = sp(batch, 0.9, lens)
    assert slow_lens == out_lens and torch.equal(slow, out)
    ident, ident_lens = sp(batch, 1.0, lens)
    assert ident_lens == lens and np.array_equal(ident.cpu().numpy(), batch)
    plan11, lens11, batch11, want11 = case((17600, 16000))
    fast, fast_lens = sp(batch11, 1.1, lens11)
    assert all(np.array_equal(bits(fast[b, :fast_lens[b]].cpu().numpy()), bits(w)) for b, w in enumerate(want11))
    with pytest.raises(ValueError):
        sp(batch, 1.2, lens)
    with pytest.raises(RuntimeError, match="rc=-3"):
        features.Resampler(16001, 16000, dev)


def write_wav(path, x, rate):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(x.astype("<i2").tobytes())


def synth(rs, n, rate, i):
    t = np.arange(n) / float(rate)
    x = 2000.0 * rs.standard_normal(n) * (0.3 + np.abs(np.sin(2 * np.pi * (1.0 + i) * t))) + 3000.0 * np.sin(2 * np.pi * (200.0 + 150.0 * i) * t)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def test_make_feat_speed_perturb_end_to_end(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    rs = np.random.RandomState(78)
    lengths = [9000, 4801, 16000, 7777, 12345, 5600]
    waves, lines, text = [], [], []
    for i, n in enumerate(lengths):
        x = synth(rs, n, 16000, i)
        path = str(tmp_path / ("utt%d.wav" % i))
        write_wav(path, x, 16000)
        waves.append(x)
        lines.append("spk_utt%d %s\n" % (i, path))
        text.append("spk_utt%d sil p%d sil\n" % (i, i))
    (tmp_path / "wav.scp").write_text("".join(lines))
    (tmp_path / "text").write_text("".join(text))
    (tmp_path / "fbank.conf").write_text("--window-type=hamming\n--num-mel-bins=40\n--dither=0\n")
    common = ["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp")]
    log = []
    _, scp = make_feat.main(common + ["--out-dir", str(tmp_path / "sp"), "--speed-perturb", "0.9,1.0,1.1", "--text", str(tmp_path / "text")], log=log.append)
    entries = [l.split() for l in open(scp)]
    keys = ["sp%s-spk_utt%d" % (f, i) for i in range(6) for f in ("0.9", "1.0", "1.1")]
    assert [e[0] for e in entries] == keys
    mats = {e[0]: read_kaldi_matrix(e[1]) for e in entries}
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf")), dev)
    sp = features.SpeedPerturb(16000, device=dev)
    for i, n in enumerate(lengths):
        for typed, f, fin in (("0.9", 0.9, 14400), ("1.0", 1.0, 16000), ("1.1", 1.1, 17600)):
            m = mats["sp%s-spk_utt%d" % (typed, i)]
            assert m.shape == (fb.num_frames(ops.resample_samples(n, fin, 16000)), 40), (i, typed)
            w, wl = sp([waves[i]], f)                                       # by hand: resample, then the filterbank
            feats, frames = fb(w, wl)
            assert int(frames[0]) == m.shape[0] and np.array_equal(feats[0, :m.shape[0]].cpu().numpy(), m), (i, typed)
    # the sp1.0- copies are the features of a run without the option
    _, scp0 = make_feat.main(common + ["--out-dir", str(tmp_path / "plain")], log=log.append)
    for e in (l.split() for l in open(scp0)):
        assert np.array_equal(read_kaldi_matrix(e[1]), mats["sp1.0-" + e[0]]), e[0]
    got_text = open(str(tmp_path / "sp" / "text")).read().splitlines()
    assert [l.split()[0] for l in got_text] == keys and all(l.split()[1:] == ["sil", "p%d" % (j // 3), "sil"] for j, l in enumerate(got_text))
    assert not os.path.exists(str(tmp_path / "plain" / "text"))
    # --compute-cmvn accumulates over all copies
    make_feat.main(common + ["--out-dir", str(tmp_path / "spc"), "--speed-perturb", "0.9,1.0,1.1", "--compute-cmvn"], log=log.append)
    stats = features.GlobalCMVN.load_kaldi_text(str(tmp_path / "spc" / "global_fbank_cmvn.txt"))
    assert int(stats.stats[0, -1]) == sum(m.shape[0] for m in mats.values())


def test_make_feat_resamples_other_rates_when_allowed(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    rs = np.random.RandomState(79)
    specs = [("hi", 44100, 20001), ("lo", 8000, 5003), ("same", 16000, 6000)]
    waves, lines = {}, []
    for i, (name, rate, n) in enumerate(specs):
        waves[name] = synth(rs, n, rate, i)
        path = str(tmp_path / (name + ".wav"))
        write_wav(path, waves[name], rate)
        lines.append("%s %s\n" % (name, path))
    (tmp_path / "wav.scp").write_text("".join(lines))
    conf = tmp_path / "fbank.conf"
    args = ["--conf", str(conf), "--wav-scp", str(tmp_path / "wav.scp"), "--out-dir", str(tmp_path / "feat")]
    conf.write_text("--num-mel-bins=40\n--dither=0\n")
    with pytest.raises(ValueError, match="44100 Hz"):
        make_feat.main(args, log=lambda s: None)
    conf.write_text("--num-mel-bins=40\n--dither=0\n--allow-downsample=true\n")
    with pytest.raises(ValueError, match="8000 Hz.*allow-upsample"):
        make_feat.main(args, log=lambda s: None)
    conf.write_text("--num-mel-bins=40\n--dither=0\n--allow-downsample=true\n--allow-upsample=true\n")
    _, scp = make_feat.main(args, log=lambda s: None)
    entries = [l.split() for l in open(scp)]
    assert [e[0] for e in entries] == ["hi", "lo", "same"]
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(conf)), dev)
    for (name, rate, n), e in zip(specs, entries):
        w, wl = features.Resampler(rate, 16000, dev)([waves[name]])
        assert wl == [ops.resample_samples(n, rate, 16000)]
        feats, frames = fb(w, wl)
        m = read_kaldi_matrix(e[1])
        assert m.shape == (int(frames[0]), 40) and m.shape[0] > 30 and np.array_equal(feats[0, :m.shape[0]].cpu().numpy(), m), name
    # a file at another rate under --speed-perturb takes one plan: round(rate f) -> the configured rate (48 510 -> 16 000 would be 1600
    # phases of 37 taps, beyond the kernel's table: the 44.1 kHz file stays out of this list)
    (tmp_path / "wav2.scp").write_text("".join(lines[1:]))
    _, scp = make_feat.main(["--conf", str(conf), "--wav-scp", str(tmp_path / "wav2.scp"), "--out-dir", str(tmp_path / "sp"), "--speed-perturb", "1.1,1.0"],
                            log=lambda s: None)
    entries = {l.split()[0]: l.split()[1] for l in open(scp)}
    assert list(entries) == ["sp1.1-lo", "sp1.0-lo", "sp1.1-same", "sp1.0-same"]
    for typed, f in (("1.1", 1.1), ("1.0", 1.0)):
        for name, rate, n in specs[1:]:
            w, wl = features.Resampler(int(round(rate * f)), 16000, dev)([waves[name]])
            feats, frames = fb(w, wl)
            m = read_kaldi_matrix(entries["sp%s-%s" % (typed, name)])
            assert m.shape[0] == int(frames[0]) and np.array_equal(feats[0, :m.shape[0]].cpu().numpy(), m), (typed, name)
