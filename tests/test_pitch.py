"""Pitch features on the MI355X (ctcn_pitch, ctcn_pitch_process; utils/features.Pitch, paste_features; steps/make_feat.py --add-pitch).

One padded batch holds every case at once: no frame, one sample short of the downsampled window, the frame that ends on the last sample,
two pitch frames against one filterbank frame, one pitch frame more than the filterbank, frame counts that cross the run length of the
walk back (plan.run) by -1, 0 and +1, once and twice over, and two utterances of about three seconds -- noise, harmonic tones, digital
silence, a constant offset, and a tone that jumps from 100 to 300 Hz half-way (long backpointer moves).  The samples are integers: the
int16 batch and the float32 batch are the same numbers, so one reference, computed once, serves both.

Parity.  Steps 4 to 7 (correlation, upsampling, Viterbi, raw output): the kernels, the host twin and tests/pitch_ref.py agree bit for bit,
the chosen lag indices included.  Step 8 (post-processing) goes through pow, exp and log: e32 = the largest difference between the float32
and the float64 restatement on the batch; the kernel stays within max(4 * e32, 1e-5) of the float64 form (the filterbank's rule)."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fbank_ref as FR  # noqa: E402
import pitch_ref as R  # noqa: E402
from ctc_pytorch_amd import ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402
from ctc_pytorch_amd.utils.data_loader import read_kaldi_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
RUN = 32                                     # frames of backpointers the walk back stages at a time (plan.run; asserted below)


def samples_for(frames):
    """Samples at 16 kHz that give exactly `frames` pitch frames under the defaults and end on the last frame's last sample."""
    return 4 * (100 + 40 * (frames - 1))


LENS = [0, 399, 400, 559, 3599] + [samples_for(t) for t in (RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, 2 * RUN + 1)] + [48000, 47999]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def tone(n, f0, amp=6000.0, rate=16000):
    return amp * R.harmonic_tone(f0, n / rate, rate)[:n].astype(np.float64)


def make_signals(lens=LENS, rate=16000, seed=31):
    rs = np.random.RandomState(seed)
    kinds = ["noise", "tone", "silence", "dc", "noisy_tone"]
    out = []
    for k, n in enumerate(lens[:-2]):
        kind = kinds[k % len(kinds)]
        if kind == "noise":
            x = 3000.0 * rs.standard_normal(n)
        elif kind == "tone":
            x = tone(n, 90.0 + 37.0 * k, rate=rate)
        elif kind == "silence":
            x = np.zeros(n)
        elif kind == "dc":
            x = np.full(n, 1234.0)
        else:
            x = tone(n, 150.0 + 11.0 * k, rate=rate) + 400.0 * rs.standard_normal(n)
        out.append(x)
    n = lens[-2]
    out.append(np.concatenate([tone(n // 2, 100.0, rate=rate), tone(n - n // 2, 300.0, rate=rate)]))     # the jump
    out.append(3000.0 * rs.standard_normal(lens[-1]))
    return [np.clip(np.round(x), -32768, 32767).astype(np.int16) for x in out]


SIGNALS = make_signals()
_REF = {}


def reference():
    """[(raw (T, 2) float32, lag indices (T))] per utterance under the defaults; computed once and shared."""
    if "raw" not in _REF:
        plan = R.Plan()
        _REF["raw"] = [R.extract(plan, s) for s in SIGNALS]
    return _REF["raw"]


def pad(signals, dtype):
    out = np.zeros((len(signals), max(max(s.shape[0] for s in signals), 1)), dtype=dtype)
    for b, s in enumerate(signals):
        out[b, :s.shape[0]] = s
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_frame_counts_of_the_batch_cover_the_edges():
    plan = ops.PitchPlan()
    assert plan.run == RUN
    got = [plan.num_frames(n) for n in LENS]
    assert got == [0, 1, 1, 2, 21, RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, 2 * RUN + 1, 298, 298]
    assert [R.fbank_frames(n) for n in LENS[:5]] == [0, 0, 1, 1, 20]            # 559 and 3599 samples: one pitch frame more


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_raw_output_equals_host_twin_and_restatement_bit_for_bit(dev, dtype):
    plan = ops.PitchPlan()
    lens = [s.shape[0] for s in SIGNALS]
    batch = torch.from_numpy(pad(SIGNALS, np.dtype(dtype))).to(dev)
    raw, frames, lags = ops.pitch(batch, lens, plan, return_lags=True)
    raw, frames, lags = raw.cpu().numpy(), frames.cpu().numpy(), lags.cpu().numpy()
    ref = reference()
    assert frames.tolist() == [r.shape[0] for r, _ in ref] == [plan.num_frames(n) for n in lens]
    assert raw.shape == (len(lens), max(frames), 2)
    for b, (want, path) in enumerate(ref):
        T = frames[b]
        assert not raw[b, T:].any() and not lags[b, T:].any(), b
        assert np.array_equal(lags[b, :T], path), (b, int((lags[b, :T] != path).sum()))
        assert same_bits(raw[b, :T], want), b
        host, host_lags = ops.pitch_host(SIGNALS[b].astype(dtype), plan, return_lags=True)
        assert same_bits(host, want) and np.array_equal(host_lags, path), b
        assert np.isfinite(raw[b]).all()
    jump = lags[len(lens) - 2, :frames[len(lens) - 2]]
    print("two-tone utterance: largest backpointer move %d states; median pitch %.1f / %.1f Hz" % (
        int(np.abs(np.diff(jump)).max()), float(np.median(raw[len(lens) - 2, 20:130, 1])), float(np.median(raw[len(lens) - 2, 170:280, 1]))))
    # 100 -> 300 Hz is log(3) / log(1.005) = 220 lag steps.  A frame's window (W + last = 182 samples) lies across the jump for at most
    # ceil(182 / 40) = 5 frames, and only those can sit between the two pitches: one move covers 220 / 5 = 44 states or more.
    assert abs(int(jump[20]) - int(jump[-20])) >= 218 and int(np.abs(np.diff(jump)).max()) >= 44
    sil = [b for b, s in enumerate(SIGNALS) if s.shape[0] and not s.any()]
    for b in sil:                                                               # digital silence: NCCF 0, the first lag (max_f0)
        assert not raw[b, :frames[b], 0].any() and (raw[b, :frames[b], 1] == np.float32(400.0)).all()


ALL_COLUMNS = dict(add_raw_log_pitch=True)


def test_post_processing_within_the_filterbank_rule(dev):
    ref = reference()
    T = max(r.shape[0] for r, _ in ref)
    raw = np.zeros((len(ref), T, 2), np.float32)
    for b, (r, _) in enumerate(ref):
        raw[b, :r.shape[0]] = r
    frames = [r.shape[0] for r, _ in ref]
    for kw in (dict(ALL_COLUMNS, delta_pitch_noise_stddev=0.0), dict(ALL_COLUMNS), dict(add_pov_feature=False, normalization_left_context=10,
                                                                                      normalization_right_context=3, delta_window=3)):
        got = ops.pitch_process(torch.from_numpy(raw).to(dev), frames, seed=5, utt_offset=2, **kw).cpu().numpy()
        e32 = ek = eh = 0.0
        for b, (r, _) in enumerate(ref):
            n = r.shape[0]
            assert not got[b, n:].any(), b
            if n == 0:
                continue
            w64, w32 = R.process(r, np.float64, seed=5, utt=2 + b, **kw), R.process(r, np.float32, seed=5, utt=2 + b, **kw)
            host = ops.pitch_process_host(r, seed=5, utt_index=2 + b, **kw)
            assert host.shape == w64.shape == got[b, :n].shape
            e32 = max(e32, float(np.abs(w32.astype(np.float64) - w64).max()))
            ek = max(ek, float(np.abs(got[b, :n].astype(np.float64) - w64).max()))
            eh = max(eh, float(np.abs(host.astype(np.float64) - w64).max()))
        print("process %s: e32 %.3g, kernel %.3g, host twin %.3g, bound %.3g" % (sorted(kw), e32, ek, eh, max(4 * e32, 1e-5)))
        assert ek <= max(4 * e32, 1e-5) and eh <= max(4 * e32, 1e-5), (kw, ek, eh, e32)


def test_noise_is_a_function_of_seed_and_utterance_index(dev):
    ref = reference()
    keep = [b for b, (r, _) in enumerate(ref) if r.shape[0] > 0]
    T = max(ref[b][0].shape[0] for b in keep)
    raw = np.zeros((len(keep), T, 2), np.float32)
    for k, b in enumerate(keep):
        raw[k, :ref[b][0].shape[0]] = ref[b][0]
    frames = [ref[b][0].shape[0] for b in keep]
    x = torch.from_numpy(raw).to(dev)
    a = ops.pitch_process(x, frames, seed=9, utt_offset=100, delta_pitch_noise_stddev=0.05)
    b2 = ops.pitch_process(x, frames, seed=9, utt_offset=100, delta_pitch_noise_stddev=0.05)
    assert torch.equal(a, b2)
    sub = ops.pitch_process(x[3:, :max(frames[3:])].contiguous(), frames[3:], seed=9, utt_offset=103, delta_pitch_noise_stddev=0.05)
    assert torch.equal(sub, a[3:, :sub.shape[1]])
    other = ops.pitch_process(x, frames, seed=10, utt_offset=100, delta_pitch_noise_stddev=0.05)
    quiet = ops.pitch_process(x, frames, seed=9, utt_offset=100, delta_pitch_noise_stddev=0.0)
    assert not torch.equal(other[:, :, 2], a[:, :, 2]) and torch.equal(other[:, :, :2], a[:, :, :2]) and torch.equal(quiet[:, :, :2], a[:, :, :2])
    g = (a[-1, :frames[-1], 2] - quiet[-1, :frames[-1], 2]).cpu().numpy().astype(np.float64) / (10.0 * 0.05)
    print("noise: mean %.3f, variance %.3f over %d frames" % (g.mean(), g.var(), g.size))
    assert abs(g.mean()) < 0.3 and 0.6 < g.var() < 1.5


def test_a_configuration_away_from_the_defaults_on_8_khz_input(dev):
    kw = dict(sample_frequency=8000.0, min_f0=60.0, max_f0=300.0, delta_pitch=0.01, resample_frequency=2000.0, lowpass_cutoff=800.0)
    plan, ref_plan = ops.PitchPlan(**kw), R.Plan(**kw)
    assert plan.num_lags == ref_plan.S and (plan.first_lag, plan.last_lag) == (ref_plan.first, ref_plan.last)
    lens = [0, 199, 200, 8000, 8000 + 4 * 20 * RUN]
    signals = make_signals(lens + [12000, 6001], rate=8000, seed=77)
    lens = [s.shape[0] for s in signals]
    raw, frames, lags = ops.pitch(torch.from_numpy(pad(signals, np.int16)).to(dev), lens, plan, return_lags=True)
    raw, frames, lags = raw.cpu().numpy(), frames.cpu().numpy(), lags.cpu().numpy()
    for b, s in enumerate(signals):
        want, path = R.extract(ref_plan, s)
        assert frames[b] == want.shape[0] == plan.num_frames(lens[b])
        assert np.array_equal(lags[b, :frames[b]], path) and same_bits(raw[b, :frames[b]], want), b
        assert not raw[b, frames[b]:].any()


def test_pitch_and_fbank_pasted_on_one_device(dev):
    fb = features.Fbank(features.FbankConfig(dither=0.0, num_mel_bins=40, window_type="hamming"), dev)
    pc = features.ProcessPitchConfig(delta_pitch_noise_stddev=0.0)
    pitch = features.Pitch(features.PitchConfig(), pc, dev)
    pick = [2, 3, 4, 6, 11]
    waves = [SIGNALS[b] for b in pick]
    base, nb = fb(waves)
    cols, npitch = pitch(waves)
    assert (npitch - nb).cpu().tolist() == [0, 1, 1, 0, 0]
    out, frames = features.paste_features(base, nb, cols, npitch)
    assert out.shape[2] == 43 and frames.tolist() == nb.cpu().tolist()
    out = out.cpu().numpy()
    o = FR.options(dither=0.0, num_mel_bins=40, window_type="hamming")
    ref = reference()
    worst = bound = 0.0
    for k, b in enumerate(pick):
        f64, f32 = FR.fbank(SIGNALS[b].astype(np.float32), o, np.float64), FR.fbank(SIGNALS[b].astype(np.float32), o, np.float32)
        p64, p32 = R.process(ref[b][0], np.float64, delta_pitch_noise_stddev=0.0), R.process(ref[b][0], np.float32, delta_pitch_noise_stddev=0.0)
        w64, w32 = R.paste(f64, p64), R.paste(f32.astype(np.float64), p32.astype(np.float64))
        assert w64.shape == (frames[k], 43)
        assert not out[k, frames[k]:].any()
        bound = max(bound, float(np.abs(w32 - w64).max()))
        worst = max(worst, float(np.abs(out[k, :frames[k]].astype(np.float64) - w64).max()))
    print("paste: e32 %.3g, kernel %.3g, bound %.3g" % (bound, worst, max(4 * bound, 1e-5)))
    assert worst <= max(4 * bound, 1e-5)
    with pytest.raises(ValueError, match="tolerance"):
        features.paste_features(base, nb, cols, npitch, length_tolerance=0)


def test_make_feat_add_pitch_end_to_end(dev, tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    from ctc_pytorch_amd.utils.data_loader import SpeechDataset
    pick = [3, 6, 11]                                                   # 559 samples: two pitch frames, one filterbank frame
    lines = []
    for i, b in enumerate(pick):
        path = str(tmp_path / ("utt%d.wav" % i))
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(SIGNALS[b].astype("<i2").tobytes())
        lines.append("utt%d %s\n" % (i, path))
    (tmp_path / "wav.scp").write_text("".join(lines))
    (tmp_path / "fbank.conf").write_text("--window-type=hamming\n--num-mel-bins=80\n--dither=0\n")
    (tmp_path / "process.conf").write_text("--delta-pitch-noise-stddev=0\n")
    common = ["--conf", str(tmp_path / "fbank.conf"), "--wav-scp", str(tmp_path / "wav.scp")]
    log = []
    _, plain_scp = make_feat.main(common + ["--out-dir", str(tmp_path / "plain")], log=log.append)
    _, scp = make_feat.main(common + ["--out-dir", str(tmp_path / "pitch"), "--add-pitch", "--pitch-process-conf", str(tmp_path / "process.conf")],
                            log=log.append)
    entries = [l.split() for l in open(scp)]
    assert [e[0] for e in entries] == ["utt0", "utt1", "utt2"]
    mats = [read_kaldi_matrix(e[1]) for e in entries]
    plain = [read_kaldi_matrix(l.split()[1]) for l in open(plain_scp)]
    fb = features.Fbank(features.FbankConfig.from_kaldi_conf(str(tmp_path / "fbank.conf")), dev)
    assert [m.shape for m in mats] == [(fb.num_frames(SIGNALS[b].shape[0]), 83) for b in pick]
    ref = reference()
    for m, p, b in zip(mats, plain, pick):
        assert np.array_equal(m[:, :80], p)                              # the base columns as they come out without --add-pitch
        want = R.process(ref[b][0], np.float64, delta_pitch_noise_stddev=0.0)[:m.shape[0]]
        assert np.abs(m[:, 80:].astype(np.float64) - want).max() <= 1e-4
    # global CMVN over the pasted matrix: 83 columns in the statistics file, every column normalised
    _, scp2 = make_feat.main(common + ["--out-dir", str(tmp_path / "cmvn"), "--add-pitch", "--compute-cmvn"], log=log.append)
    stats = features.GlobalCMVN.load_kaldi_text(str(tmp_path / "cmvn" / "global_fbank_cmvn.txt"))
    allf = np.concatenate([read_kaldi_matrix(l.split()[1]) for l in open(scp2)]).astype(np.float64)
    assert stats.feat_dim == 83 and int(stats.stats[0, 83]) == allf.shape[0] == sum(m.shape[0] for m in mats)
    print("make_feat --add-pitch --compute-cmvn: max |mean| %.3g, max |var - 1| %.3g" % (np.abs(allf.mean(0)).max(), np.abs(allf.var(0) - 1).max()))
    assert np.abs(allf.mean(axis=0)).max() <= 1e-3 and np.abs(allf.var(axis=0) - 1.0).max() <= 1e-2
    # the archive flows through the loader
    from ctc_pytorch_amd.utils.data_loader import SpeechDataLoader, Vocab

    class Opts(object):
        left_ctx, right_ctx, n_skip_frame, n_downsample = 0, 0, 1, 1

    (tmp_path / "text").write_text("".join("utt%d a b c\n" % i for i in range(3)))
    (tmp_path / "units").write_text("a\nb\nc\n")
    batches = list(SpeechDataLoader(SpeechDataset(Vocab(str(tmp_path / "units")), scp, str(tmp_path / "text"), Opts), batch_size=3, shuffle=False))
    assert len(batches) == 1 and batches[0][0].shape[0] == 3 and batches[0][0].shape[2] == 83
