"""Pitch features, the host side, without a GPU: the plan (ctcn_pitch_plan) against the restatement of tests/pitch_ref.py bit for bit, the
refusals, the frame counts, the host twin (ctcn_pitch_host, the kernels' arithmetic) bit for bit against the restatement, the definition's
sanity on harmonic tones, the post-processing twin within the filterbank's rule (e32 = the largest difference between the float32 and the
float64 restatement; the twin stays within max(4 * e32, 1e-5) of the float64 form), paste_features' length rule and make_feat.py's
argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as R  # noqa: E402
from ctc_pytorch_amd import ops  # noqa: E402
from ctc_pytorch_amd.steps import make_feat  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_plan(plan, ref):
    assert (plan.num_lags, plan.first_lag, plan.last_lag, plan.window, plan.shift) == (ref.S, ref.first, ref.last, ref.W, ref.shift)
    assert same_bits(plan.lags, ref.lags) and same_bits(plan.pitch, ref.pitch)
    assert same_bits(plan.soft_lag, ref.soft_lag) and same_bits(plan.penalty, ref.penalty)
    assert np.array_equal(plan.tap_first, ref.tap_first) and np.array_equal(plan.tap_count, ref.tap_count)
    assert plan.stride == ref.taps and same_bits(plan.weights, ref.weights)


def test_plan_equals_the_restatement_bit_for_bit():
    plan, ref = ops.PitchPlan(), R.Plan()
    assert plan.num_lags == 417 and (plan.first_lag, plan.last_lag) == (8, 82) and (plan.window, plan.shift) == (100, 40)
    assert plan.stride <= 11 and plan.run >= 1
    check_plan(plan, ref)
    assert plan.lags[0] == np.float32(1.0 / 400.0) and plan.lags[-1] <= np.float32(1.0 / 50.0) < np.float32(np.float64(plan.lags[-1]) * 1.005)
    assert plan.penalty[0] == 0.0 and abs(plan.penalty[416] - 0.43) < 0.01        # a jump across every state costs 0.43
    # every row of the upsampling table is a partition of (nearly) one: a constant row stays a constant away from the clipped edges
    inner = (plan.tap_first > 0) & (plan.tap_first + plan.tap_count < plan.last_lag - plan.first_lag + 1)
    assert inner.sum() > 300 and np.abs(plan.weights[inner].astype(np.float64).sum(axis=1) - 1.0).max() < 0.02
    for kw in (dict(sample_frequency=8000.0, min_f0=60.0, max_f0=300.0, delta_pitch=0.01, resample_frequency=2000.0, lowpass_cutoff=800.0),
               dict(upsample_filter_width=3, soft_min_f0=20.0, penalty_factor=0.3, frame_length=30.0, frame_shift=5.0)):
        check_plan(ops.PitchPlan(**kw), R.Plan(**kw))


def test_refusals_come_from_the_plan_builder():
    for kw in (dict(snip_edges=False), dict(delta_pitch=0.0005), dict(min_f0=400.0), dict(min_f0=500.0), dict(lowpass_cutoff=2001.0),
               dict(sample_frequency=2000.0, resample_frequency=4000.0, lowpass_cutoff=1001.0), dict(preemphasis_coefficient=0.97),
               dict(resample_frequency=4000.5), dict(upsample_filter_width=0)):
        with pytest.raises(RuntimeError, match="rc=-3"):
            ops.PitchPlan(**kw)
    assert ops.PitchPlan(delta_pitch=0.0021).num_lags <= 1024                    # 991 lags: the largest table the search takes
    with pytest.raises(ValueError, match="unknown option"):
        ops.PitchPlan(frames_per_chunk=10)
    raw = np.array([[0.5, 100.0], [0.6, 110.0]], np.float32)
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.pitch_process_host(raw, delay=1)
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.pitch_process_host(raw, delta_window=6)
    with pytest.raises(ValueError, match="switched off"):
        ops.pitch_process_host(raw, add_pov_feature=False, add_normalized_log_pitch=False, add_delta_pitch=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pitch(torch.zeros(1, 400), [400], ops.PitchPlan())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pitch_process(torch.zeros(1, 2, 2), [2])
    with pytest.raises(TypeError, match="PitchPlan"):
        ops.pitch_frames(400, None)


def test_frame_counts():
    plan, ref = ops.PitchPlan(), R.Plan()
    lens = [0, 399, 400, 403, 404, 559, 560, 561]
    assert [ops.pitch_frames(n, plan) for n in lens] == [ref.num_frames(n) for n in lens] == [0, 1, 1, 1, 1, 2, 2, 2]
    assert [ops.fbank_frames(n, 400, 160) for n in lens] == [0, 0, 1, 1, 1, 1, 2, 2]
    for n in range(0, 3000, 7):
        assert ops.pitch_frames(n, plan) == ref.num_frames(n)
        assert 0 <= ops.pitch_frames(n, plan) - ops.fbank_frames(n, 400, 160) <= 1
    with pytest.raises(ValueError):
        ops.pitch_frames(-1, plan)


def signals():
    rs = np.random.RandomState(5)
    t = np.arange(9000)
    return {
        "noise": (3000.0 * rs.standard_normal(8000)).astype(np.float32),
        "tone": (6000.0 * R.harmonic_tone(140.0, 0.5)).astype(np.float32),
        "silence": np.zeros(4000, np.float32),
        "dc": np.full(4000, 2500.0, np.float32),
        "int16_full_scale": np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16),
        "one_frame": (3000.0 * rs.standard_normal(401)).astype(np.float32),
        "no_frame": (3000.0 * rs.standard_normal(396)).astype(np.float32),          # 99 downsampled samples: one short of the window
        "unit_scale": rs.standard_normal(3000).astype(np.float32) * np.float32(0.1),
    }


def test_host_twin_equals_the_restatement_bit_for_bit():
    plan, ref = ops.PitchPlan(), R.Plan()
    for name, x in signals().items():
        got, lags = ops.pitch_host(x, plan, return_lags=True)
        want, path = R.extract(ref, x)
        assert got.shape == (ref.num_frames(x.shape[0]), 2), name
        assert np.array_equal(lags, path), (name, int((lags != path).sum()))
        assert same_bits(got, want), name
        assert np.isfinite(got).all(), name
        if name == "silence":                                          # every correlation 0: ties everywhere, the lowest index wins
            assert not got[:, 0].any() and (got[:, 1] == np.float32(400.0)).all() and not lags.any()
        if name == "one_frame":
            assert got.shape[0] == 1
        if name == "no_frame":
            assert got.shape[0] == 0
    kw = dict(sample_frequency=8000.0, min_f0=60.0, max_f0=300.0, delta_pitch=0.01, resample_frequency=2000.0, lowpass_cutoff=800.0)
    x = (5000.0 * R.harmonic_tone(97.0, 0.6, rate=8000)).astype(np.float32)
    got, lags = ops.pitch_host(x, ops.PitchPlan(**kw), return_lags=True)
    want, path = R.extract(R.Plan(**kw), x)
    assert same_bits(got, want) and np.array_equal(lags, path)


def test_the_definition_finds_the_pitch_of_harmonic_tones():
    plan = ops.PitchPlan()
    for f0 in (80.0, 120.0, 220.0, 330.0):
        raw = ops.pitch_host(R.harmonic_tone(f0), plan)
        mid = raw[5:-5]
        pitch, nccf = float(np.median(mid[:, 1])), float(np.median(mid[:, 0]))
        print("tone %5.1f Hz: median pitch %.2f Hz, median NCCF %.4f over %d frames" % (f0, pitch, nccf, mid.shape[0]))
        assert abs(pitch - f0) <= 0.01 * f0 and nccf > 0.99
    noise = np.random.RandomState(1).standard_normal(16000).astype(np.float32)
    nccf = float(np.median(ops.pitch_host(noise, plan)[5:-5, 0]))
    print("white noise: median NCCF %.3f" % nccf)
    assert nccf < 0.6


def _raw(T, seed):
    rs = np.random.RandomState(seed)
    raw = np.zeros((T, 2), np.float32)
    raw[:, 0] = np.clip(0.5 + 0.5 * rs.standard_normal(T), -1.02, 1.02)            # beyond +-1 too: the clips
    raw[:, 1] = np.float32(1.0) / ops.PitchPlan().lags[rs.randint(0, 417, T)]
    return raw


PROCESS_CASES = [dict(), dict(delta_pitch_noise_stddev=0.0), dict(add_raw_log_pitch=True), dict(add_pov_feature=False),
                 dict(add_normalized_log_pitch=False), dict(add_delta_pitch=False, add_raw_log_pitch=True),
                 dict(normalization_left_context=10, normalization_right_context=0, delta_window=1, pov_offset=0.5, pitch_scale=1.0),
                 dict(delta_pitch_noise_stddev=0.1, delta_window=5, pov_scale=1.0, delta_pitch_scale=3.0)]


def test_post_processing_twin_within_the_filterbank_rule():
    worst = 0.0
    for T in (0, 1, 2, 75, 76, 151, 152, 400):           # the window of 75 + 1 + 75 frames clipped on both sides, on one, on none
        raw = _raw(T, T)
        for k, kw in enumerate(PROCESS_CASES if T in (2, 152) else PROCESS_CASES[:3]):
            got = ops.pitch_process_host(raw, seed=11, utt_index=k, **kw)
            w64, w32 = R.process(raw, np.float64, seed=11, utt=k, **kw), R.process(raw, np.float32, seed=11, utt=k, **kw)
            cols = sum(bool(dict(R.PROCESS_OPTS, **kw)[c]) for c in ("add_pov_feature", "add_normalized_log_pitch", "add_delta_pitch", "add_raw_log_pitch"))
            assert got.dtype == np.float32 and got.shape == w64.shape == (T, cols), (T, kw)
            if T == 0:
                continue
            e32 = float(np.abs(w32.astype(np.float64) - w64).max())
            ek = float(np.abs(got.astype(np.float64) - w64).max())
            worst = max(worst, ek)
            assert ek <= max(4 * e32, 1e-5), (T, kw, ek, e32)
            assert np.isfinite(got).all()
    print("post-processing twin: largest difference to the float64 restatement %.3g" % worst)
    raw = _raw(40, 3)
    a = ops.pitch_process_host(raw, seed=1, utt_index=4, delta_pitch_noise_stddev=0.05)
    assert same_bits(a, ops.pitch_process_host(raw, seed=1, utt_index=4, delta_pitch_noise_stddev=0.05))
    b = ops.pitch_process_host(raw, seed=1, utt_index=5, delta_pitch_noise_stddev=0.05)
    assert same_bits(a[:, :2], b[:, :2]) and not np.array_equal(a[:, 2], b[:, 2])
    # one frame: its own window, so the normalised log pitch is 0 and the delta of a constant is 0
    one = ops.pitch_process_host(_raw(1, 9), delta_pitch_noise_stddev=0.0)
    assert abs(one[0, 1]) < 1e-6 and abs(one[0, 2]) < 1e-6


def test_configs_read_kaldi_files(tmp_path):
    (tmp_path / "pitch.conf").write_text("--min-f0=60\n--max-f0=300  # a comment\n--delta-pitch=0.01\n--snip-edges=true\n")
    c = features.PitchConfig.from_kaldi_conf(str(tmp_path / "pitch.conf"))
    assert (c.min_f0, c.max_f0, c.delta_pitch, c.snip_edges, c.resample_frequency) == (60.0, 300.0, 0.01, True, 4000.0)
    assert c.plan().num_lags == R.Plan(min_f0=60.0, max_f0=300.0, delta_pitch=0.01).S
    (tmp_path / "process.conf").write_text("--add-raw-log-pitch\n--delta-pitch-noise-stddev=0\n--normalization-left-context=50\n")
    p = features.ProcessPitchConfig.from_kaldi_conf(str(tmp_path / "process.conf"))
    assert p.feat_dim == 4 and p.delta_pitch_noise_stddev == 0.0 and p.normalization_left_context == 50 and p.delay == 0
    assert features.ProcessPitchConfig().feat_dim == 3
    (tmp_path / "bad.conf").write_text("--frames-per-chunk=10\n")
    with pytest.raises(ValueError, match="unknown or unsupported"):
        features.PitchConfig.from_kaldi_conf(str(tmp_path / "bad.conf"))
    with pytest.raises(ValueError, match="unknown option"):
        features.ProcessPitchConfig(max_frames_latency=3)
    with pytest.raises(RuntimeError, match="rc=-3"):
        features.PitchConfig(snip_edges=False).plan()
    with pytest.raises(RuntimeError, match="delay"):
        features.Pitch(features.PitchConfig(), features.ProcessPitchConfig(delay=2), "cpu")


def test_paste_features_length_rule():
    rs = np.random.RandomState(2)
    a, b = torch.from_numpy(rs.standard_normal((3, 9, 4)).astype(np.float32)), torch.from_numpy(rs.standard_normal((3, 10, 3)).astype(np.float32))
    out, frames = features.paste_features(a, [9, 5, 0], b, [9, 6, 2])                       # equal, one apart, two apart
    assert frames.tolist() == [9, 5, 0] and out.shape == (3, 9, 7)
    for i, n in enumerate(frames.tolist()):
        want = R.paste(a[i, :[9, 5, 0][i]].numpy(), b[i, :[9, 6, 2][i]].numpy())
        assert np.array_equal(out[i, :n].numpy(), want) and not out[i, n:].any()
    out2, frames2 = features.paste_features(b, torch.tensor([9, 6, 2]), a, torch.tensor([9, 5, 0]))
    assert frames2.tolist() == [9, 5, 0] and torch.equal(out2[:, :, :3], out[:, :, 4:]) and torch.equal(out2[:, :, 3:], out[:, :, :4])
    with pytest.raises(ValueError, match="tolerance"):
        features.paste_features(a, [9, 5, 0], b, [9, 6, 3])                                 # three apart
    with pytest.raises(ValueError, match="differ by more than 2"):
        R.paste(np.zeros((0, 4)), np.zeros((3, 3)))
    features.paste_features(a, [9, 5, 0], b, [9, 6, 3], length_tolerance=3)
    with pytest.raises(ValueError, match="tolerance"):
        features.paste_features(a, [9, 5, 0], b, [9, 6, 0], length_tolerance=0)
    with pytest.raises(ValueError):
        features.paste_features(a, [9, 5], b, [9, 6, 2])


def test_make_feat_arguments():
    base = ["--conf", "fbank.conf", "--wav-scp", "wav.scp", "--out-dir", "out"]
    plain = make_feat.parse_args(base)
    assert plain.add_pitch is False and plain.pitch_conf is None and plain.pitch_process_conf is None and plain.paste_length_tolerance is None
    args = make_feat.parse_args(base + ["--add-pitch", "--pitch-conf", "p.conf", "--pitch-process-conf", "q.conf", "--paste-length-tolerance", "1",
                                        "--feat-type", "mfcc", "--speed-perturb", "0.9,1.0,1.1", "--cmvn-per-utt"])
    assert args.add_pitch and args.pitch_conf == "p.conf" and args.pitch_process_conf == "q.conf" and args.paste_length_tolerance == 1
    with pytest.raises(ValueError, match="logspec"):
        make_feat.parse_args(base + ["--add-pitch", "--feat-type", "logspec"])
    for extra in (["--pitch-conf", "p.conf"], ["--pitch-process-conf", "q.conf"], ["--paste-length-tolerance", "2"]):
        with pytest.raises(ValueError, match="belongs to --add-pitch"):
            make_feat.parse_args(base + extra)
    with pytest.raises(ValueError, match="count of frames"):
        make_feat.parse_args(base + ["--add-pitch", "--paste-length-tolerance", "-1"])
