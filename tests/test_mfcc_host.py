"""Host-side checks of the MFCC front-end (no GPU): the plan builder (the filterbank plan bit for bit, then the DCT table and the lifter
against tests/mfcc_ref.py), its refusals, the Kaldi config reader under MFCC defaults, the driver's --feat-type and the restatement itself.

Bounds.  DCT table and lifter: both sides evaluate one double expression and round once to float32; cos / sin of two maths libraries may
differ in the last place of the double, which can move the rounding by one float32 ulp."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fbank_ref as R  # noqa: E402
import mfcc_ref as MR  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulps(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    key = lambda a: np.where(a.view(np.int32) < 0, np.int64(-2 ** 31) - a.view(np.int32).astype(np.int64), a.view(np.int32).astype(np.int64))
    return int(np.abs(key(got) - key(want)).max())       # sign-magnitude -> monotone integers: a distance across zero counts too


@pytest.mark.parametrize("N,C,Q,extra", [(23, 13, 22.0, {}), (40, 20, 22.0, {}), (80, 64, 0.0, {}), (23, 23, 22.0, {}),
                                         (128, 64, 22.0, dict(frame_length=50.0))])
def test_plan_is_the_filterbank_plan_then_table_and_lifter(N, C, Q, extra):
    cfg = features.MfccConfig(num_mel_bins=N, num_ceps=C, cepstral_lifter=Q, **extra)
    plan = ops.MfccPlan(cfg.c_opts())
    npad = plan.padded_length
    assert npad == (1024 if extra else 512) and plan.feat_dim == cfg.feat_dim == C and plan.num_ceps == C
    head = 6 * npad + 384
    assert plan.host.size == head + N * C + C
    assert _lib.lib().ctcn_mfcc_plan_bytes(ctypes.byref(cfg.c_opts())) == 4 * plan.host.size
    for use_energy in (False, True):                                    # the filterbank's plan does not depend on it
        fb = ops.FbankPlan(features.FbankConfig(num_mel_bins=N, use_energy=use_energy, **extra).c_opts())
        assert fb.host.size == head and np.array_equal(plan.host[:head], fb.host)
    f32 = plan.host.view(np.float32)
    table = f32[head:head + N * C].reshape(N, C)                        # bin-major: D[k][n] at word n * C + k
    want = MR.dct_matrix(N, C).astype(np.float32)
    assert ulps(np.ascontiguousarray(table.T), want) <= 1
    if C < N:
        assert ulps(np.ascontiguousarray(f32[head:head + N * C].reshape(C, N)), want) > 1000      # (the ceps-major reading is another matrix)
    assert np.array_equal(table[:, 0], np.full(N, np.float32(np.sqrt(1.0 / N))))
    lift = f32[head + N * C:]
    assert ulps(lift, MR.lifter(C, Q).astype(np.float32)) <= 1
    if Q == 0:
        assert np.array_equal(lift, np.ones(C, dtype=np.float32))
    else:
        assert lift[0] == 1.0 and abs(float(lift[1]) - (1.0 + 11.0 * np.sin(np.pi / 22.0))) < 1e-6


def test_plan_refuses_before_any_launch():
    L = _lib.lib()
    for kw, code in ((dict(num_ceps=0), -1), (dict(num_ceps=24), -1), (dict(cepstral_lifter=-1.0), -1),
                     (dict(num_mel_bins=80, num_ceps=65), -3),
                     (dict(frame_length=100.0), -3), (dict(num_mel_bins=129), -3), (dict(round_to_power_of_two=False), -3),
                     (dict(num_mel_bins=2, num_ceps=2), -1), (dict(low_freq=9000.0), -1)):
        cfg = features.MfccConfig(**kw)
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            ops.MfccPlan(cfg.c_opts())
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            features.Mfcc(cfg, "cpu")
        if "low_freq" not in kw:                                        # (the bank's frequency check belongs to the builder, not to the geometry)
            assert L.ctcn_mfcc_plan_bytes(ctypes.byref(cfg.c_opts())) == 0, kw
    assert ops.MfccPlan(features.MfccConfig(num_mel_bins=80, num_ceps=64).c_opts()).feat_dim == 64
    o = features.MfccConfig().c_opts()
    assert L.ctcn_mfcc_plan(ctypes.byref(o), None, 0) == -1 and L.ctcn_mfcc_plan(None, None, 0) == -1 and L.ctcn_mfcc_plan_bytes(None) == 0
    small = np.zeros(16, dtype=np.uint32)
    assert L.ctcn_mfcc_plan(ctypes.byref(o), small.ctypes.data_as(ctypes.c_void_p), small.nbytes) == -1 and not small.any()


def test_kaldi_conf_reader_with_mfcc_defaults(tmp_path):
    d = features.MfccConfig.DEFAULTS
    assert d == MR.DEFAULTS and d["use_energy"] is True and (d["num_mel_bins"], d["num_ceps"], d["cepstral_lifter"]) == (23, 13, 22.0)
    assert "use_log_fbank" not in d and "use_power" not in d
    assert features.FbankConfig.DEFAULTS == R.DEFAULTS                  # the filterbank's are untouched
    conf = tmp_path / "mfcc.conf"
    conf.write_text("--use-energy=false   # only non-default option.\n")          # the reference's conf/mfcc.conf
    c = features.MfccConfig.from_kaldi_conf(str(conf))
    assert c.use_energy is False and c.feat_dim == 13
    assert all(getattr(c, k) == v for k, v in d.items() if k != "use_energy")
    conf.write_text("--use-power=false\n")
    with pytest.raises(ValueError, match="use-power"):
        features.MfccConfig.from_kaldi_conf(str(conf))
    conf.write_text("--use-log-fbank=true\n")
    with pytest.raises(ValueError, match="use-log-fbank"):
        features.MfccConfig.from_kaldi_conf(str(conf))
    with pytest.raises(ValueError, match="MfccConfig: unknown option 'use_power'"):
        features.MfccConfig(use_power=False)
    conf.write_text("--num-ceps=20 --cepstral-lifter=0 --htk-compat\n".replace(" --", "\n--"))
    c = features.MfccConfig.from_kaldi_conf(str(conf))
    assert (c.num_ceps, c.cepstral_lifter, c.htk_compat, c.use_energy, c.feat_dim) == (20, 0.0, True, True, 20)
    o = c.c_opts()
    assert (o.num_ceps, o.cepstral_lifter, o.htk_compat, o.use_energy, o.num_mel_bins, o.window_type) == (20, 0.0, 1, 1, 23, 2)
    conf.write_text("--num-ceps=13\n")                                  # an MFCC key is no filterbank key
    with pytest.raises(ValueError, match="num-ceps"):
        features.FbankConfig.from_kaldi_conf(str(conf))


def test_ops_mfcc_raises_for_cpu_tensors_and_foreign_plans():
    plan = ops.MfccPlan(features.MfccConfig().c_opts())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mfcc(torch.zeros(1, 400), [400], plan)
    with pytest.raises(ValueError, match=r"ctc_pytorch_amd.mfcc: expected wave \(B, Nmax\)"):
        ops.mfcc(torch.zeros(400), [400], plan)
    fb = ops.FbankPlan(features.FbankConfig().c_opts())
    with pytest.raises(TypeError, match="MfccPlan"):                    # the two plans carry different option structs
        ops.mfcc(torch.zeros(1, 400), [400], fb)
    with pytest.raises(TypeError, match="FbankPlan"):
        ops.fbank(torch.zeros(1, 400), [400], plan)


def test_make_feat_help_lists_feat_type():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "ctc_pytorch_amd", "steps", "make_feat.py"), "--help"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "--feat-type" in p.stdout and "mfcc" in p.stdout and "--compute-cmvn" in p.stdout, p.stderr[-400:]


def test_restatement_by_hand():
    """One cepstrum from the plain cosine sum over fbank_ref's float64 log-mel row; the energy column; the HTK order; float32 follows float64."""
    x = np.round(3000.0 * np.random.RandomState(1).standard_normal(4000))
    o = MR.options(dither=0.0)
    c = MR.mfcc(x, o, np.float64)
    fb = R.fbank(x, R.options(dither=0.0, use_energy=True), np.float64)
    assert c.shape == (23, 13) and fb.shape == (23, 24)
    assert np.array_equal(c[:, 0], fb[:, 0])                            # use_energy: column 0 is the filterbank's energy column
    t, k, N, Q = 5, 7, 23, 22.0
    m = fb[t, 1:]
    by_hand = sum(np.sqrt(2.0 / N) * np.cos(np.pi / N * (n + 0.5) * k) * m[n] for n in range(N)) * (1.0 + 0.5 * Q * np.sin(np.pi * k / Q))
    assert abs(c[t, k] - by_hand) <= 1e-12
    # C0 without energy: the lifter is 1 there; sqrt(1 / N) times the sum of the log-mels
    c0 = MR.mfcc(x, MR.options(dither=0.0, use_energy=False), np.float64)
    assert abs(c0[t, 0] - m.sum() / np.sqrt(N)) <= 1e-12 and np.abs(c0[:, 1:] - c[:, 1:]).max() == 0.0
    # HTK: C0 * sqrt 2 (or the energy) in the last column, the others down by one; the bank's first-bin quirk moves only the lowest filter
    h = MR.mfcc(x, MR.options(dither=0.0, use_energy=False, htk_compat=True), np.float64)
    fbh = R.fbank(x, R.options(dither=0.0, htk_compat=True), np.float64)
    assert abs(h[t, 12] - np.sqrt(2.0) * fbh[t].sum() / np.sqrt(N)) <= 1e-12
    want = sum(np.sqrt(2.0 / N) * np.cos(np.pi / N * (n + 0.5) * 3) * fbh[t, n] for n in range(N)) * (1.0 + 0.5 * Q * np.sin(np.pi * 3 / Q))
    assert abs(h[t, 2] - want) <= 1e-12
    he = MR.mfcc(x, MR.options(dither=0.0, htk_compat=True), np.float64)
    assert np.array_equal(he[:, 12], fb[:, 0]) and np.array_equal(he[:, :12], h[:, :12])
    # no lifter
    nl = MR.mfcc(x, MR.options(dither=0.0, cepstral_lifter=0.0), np.float64)
    assert np.abs(nl[:, 1:] * MR.lifter(13, 22.0)[None, 1:] - c[:, 1:]).max() <= 1e-12
    # the float32 chain follows (grossly here: its true distance is what the GPU test measures as e32)
    c32 = MR.mfcc(x, o, np.float32)
    assert c32.dtype == np.float32 and np.abs(c32 - c).max() < 1e-2
