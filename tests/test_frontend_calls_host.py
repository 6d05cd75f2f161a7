"""The arguments the front-end wrappers hand to the device entry points of the C ABI, without a GPU: the wrappers run on CPU tensors against a
recorder around the real library -- host-only entries (plans, frame counts, limits, workspace sizes, the host twins) pass through, the
fourteen device entries are recorded and answer 0 -- and every record is compared, exactly, with tests/golden/frontend_calls.json.  One record
holds the entry's name and per argument "null" / "ptr" for a pointer ("stream" for the stream), the value of an int or a float and the fields
of a struct passed by reference; a case also records the workspace requests and the shapes and dtypes of what the wrapper returned.

The golden file was recorded from the wrappers as they stood in ops.py before they moved to frontend.py, by this test body.  To record it
again run this file with CTCN_RECORD_FRONTEND_CALLS=1: the test then writes the file and fails, so that a recording run is never taken for a
comparison.  The same file holds the surface check: every public front-end name is the same object on ops and on frontend."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from ctc_pytorch_amd import _lib, ops
from ctc_pytorch_amd.utils import features

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_calls.json")
RECORD = "CTCN_RECORD_FRONTEND_CALLS"
DEVICE_ENTRIES = ("ctcn_fbank", "ctcn_mfcc", "ctcn_spectrogram", "ctcn_logspec", "ctcn_resample", "ctcn_frame_context", "ctcn_spec_augment",
                  "ctcn_reverb", "ctcn_cmvn_accumulate", "ctcn_cmvn_accumulate_groups", "ctcn_cmvn_apply", "ctcn_cmvn_sliding", "ctcn_pitch",
                  "ctcn_pitch_process")
PUBLIC = ["fbank_frames", "FbankPlan", "MfccPlan", "SpectrogramPlan", "fbank", "mfcc", "spectrogram", "LogSpecPlan", "log_spectrum",
          "resample_samples", "ResamplePlan", "resample", "context_frames", "delta_scales", "frame_context_tile", "frame_context",
          "SPEC_AUGMENT_OPTIONS", "spec_augment_plan", "spec_augment_host", "spec_augment", "REVERB_LIMIT_FIELDS", "reverb_limits", "ReverbBank",
          "reverb_plan", "reverberate_host", "reverberate", "cmvn_accumulate", "_cmvn_groups", "cmvn_accumulate_groups", "cmvn_apply",
          "cmvn_sliding_run", "cmvn_sliding_window", "cmvn_sliding_host", "cmvn_norm_host", "cmvn_sliding", "PITCH_OPTIONS",
          "PITCH_PROCESS_OPTIONS", "PitchPlan", "pitch_frames", "pitch", "pitch_host", "pitch_process", "pitch_process_host",
          "CONTEXT_OPTIONS", "REVERB_OPTIONS", "SLIDING_CMN_OPTIONS"]
STREAM = 0x57AE                     # what the patched stream_ptr answers: recorded as "stream"


def _arg(a, argtype):
    if argtype is ctypes.c_void_p:
        if hasattr(a, "_obj"):                                          # ctypes.byref(struct)
            return {k: getattr(a._obj, k) for k, _ in a._obj._fields_}
        if a == STREAM and isinstance(a, int):
            return "stream"
        if a is None or (isinstance(a, ctypes.c_void_p) and not a.value):
            return "null"
        return "ptr"
    return float(a) if argtype in (ctypes.c_float, ctypes.c_double) else int(a)


class _Recorder(object):
    """The library as the wrappers see it: device entries are logged and answer 0, everything else is the real library's."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in DEVICE_ENTRIES:
            return fn

        def entry(*args):
            assert len(args) == len(fn.argtypes), name
            self._log.append({"entry": name, "args": [_arg(a, t) for a, t in zip(args, fn.argtypes)]})
            return 0
        return entry


def _returned(x):
    if torch.is_tensor(x):
        return {"shape": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, (list, tuple)):
        return [_returned(v) for v in x]
    return x


@pytest.fixture
def run(monkeypatch):
    """run(fn, *args, **kw) -> {"calls": [...], "returned": ...} with the library, the workspace, the stream and the device check replaced."""
    log = []
    real = _lib.lib()
    home = sys.modules[ops.fbank.__module__]                             # the module the wrappers live in

    def workspace(device, nbytes=None, tag="main"):
        log.append({"workspace": tag, "nbytes": int(nbytes)})
        return torch.empty(int(nbytes), dtype=torch.uint8)

    monkeypatch.setattr(_lib, "lib", lambda: _Recorder(real, log))
    monkeypatch.setattr(_lib, "workspace", workspace)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(_lib, "_need_gpu", lambda *ts: None, raising=False)
    monkeypatch.setattr(home, "_need_gpu", lambda *ts: None)

    def one(fn, *args, **kw):
        del log[:]
        out = fn(*args, **kw)
        return {"calls": list(log), "returned": _returned(out)}
    return one


def _waves(dtype, lens=(700, 0), nmax=800):
    rs = np.random.RandomState(3)
    w = (3000.0 * rs.standard_normal((len(lens), nmax))).astype(np.float32)
    return torch.from_numpy(w.astype(np.int16) if dtype == "int16" else w), list(lens)


def _feats(B=2, T=9, F=5):
    return torch.from_numpy(np.random.RandomState(5).standard_normal((B, T, F)).astype(np.float32))


def _features_cases(run):
    got = {}
    f32, lens = _waves("float32")
    i16, _ = _waves("int16")
    short, short_lens = _waves("float32", lens=(100, 0), nmax=120)       # fewer samples than one frame: Tmax = 0
    fb = ops.FbankPlan(features.FbankConfig(num_mel_bins=8, use_energy=True).c_opts())
    mf = ops.MfccPlan(features.MfccConfig(num_mel_bins=10, num_ceps=6).c_opts())
    sp = ops.SpectrogramPlan(features.SpectrogramConfig(frame_length=20.0, snip_edges=False).c_opts())
    ls = ops.LogSpecPlan(features.LogSpecConfig(window_size=0.016, window_stride=0.008, normalize=False).c_opts())
    for name, op, plan in (("fbank", ops.fbank, fb), ("mfcc", ops.mfcc, mf), ("spectrogram", ops.spectrogram, sp)):
        F = plan.feat_dim
        got[name + " float32, host lengths"] = run(op, f32, lens, plan)
        got[name + " int16, tensor lengths, mean and scale, dither, seed, offset"] = run(
            op, i16, torch.tensor(lens), plan, mean=torch.zeros(F), scale=torch.ones(F), dither=0.5, seed=-3, utt_offset=7)
        got[name + " lengths beyond Nmax and below 0"] = run(op, f32, [900, -4], plan, seed=(1 << 64) + 5)
        if plan.snip_edges:
            got[name + " Tmax 0"] = run(op, short, short_lens, plan)
    got["log_spectrum float32, host lengths"] = run(ops.log_spectrum, f32, lens, ls)
    got["log_spectrum int16, tensor lengths"] = run(ops.log_spectrum, i16, torch.tensor(lens, dtype=torch.int64), ls)
    got["log_spectrum all lengths 0"] = run(ops.log_spectrum, f32, [0, 0], ls)
    return got


def _resample_cases(run):
    got = {}
    f32, lens = _waves("float32")
    i16, _ = _waves("int16")
    down = ops.ResamplePlan(16000, 8000)
    up = ops.ResamplePlan(16000, 17600, num_zeros=4, cutoff=7000.0)
    got["resample float32, host lengths"] = run(ops.resample, f32, lens, down)
    got["resample int16, tensor lengths, other plan"] = run(ops.resample, i16, torch.tensor(lens), up)
    got["resample Mmax 0"] = run(ops.resample, f32, [0, -2], down)
    got["resample lengths beyond Nmax"] = run(ops.resample, f32, [801, 3], down)
    return got


def _context_cases(run):
    got = {}
    x = _feats()
    got["frame_context defaults, host frames"] = run(ops.frame_context, x, [9, 0])
    got["frame_context options, tensor frames"] = run(ops.frame_context, x, torch.tensor([4, 9]), left=2, right=1, skip=2, n_downsample=4,
                                                      delta_order=2, delta_window=3)
    got["frame_context positional options"] = run(ops.frame_context, x, [9, 12], 1, 0, 3, 1, 1, 1)
    got["frame_context Tin_max 0"] = run(ops.frame_context, torch.zeros(2, 0, 5), [0, 0], left=1)
    got["spec_augment defaults, host frames"] = run(ops.spec_augment, x, [9, 0], 11)
    got["spec_augment options, tensor frames"] = run(ops.spec_augment, x, torch.tensor([4, 9]), -2, utt_offset=-1, warp_window=3,
                                                     num_freq_masks=2, freq_width=2, num_time_masks=1, time_width=4, time_ratio=0.5, fill=-1.5)
    got["spec_augment Tmax 0"] = run(ops.spec_augment, torch.zeros(2, 0, 5), [0, 0], 1 << 64, utt_offset=(1 << 64) + 9)
    return got


def _reverb_cases(run):
    got = {}
    f32, lens = _waves("float32")
    i16, _ = _waves("int16")
    rs = np.random.RandomState(9)
    rirs = [rs.standard_normal(40).astype(np.float32), rs.standard_normal(64).astype(np.float32)]
    noises = [(100.0 * rs.standard_normal(300)).astype(np.float32)]
    bank = ops.ReverbBank(rirs, noises, 16000.0, snrs=(20, 5))
    dry = ops.ReverbBank([], noises, 16000.0)
    got["reverberate float32, host lengths"] = run(ops.reverberate, f32, lens, bank, 5)
    got["reverberate int16, tensor lengths, options"] = run(ops.reverberate, i16, torch.tensor(lens), bank, -1, utt_offset=-2, rir_prob=0.25,
                                                            noise_prob=0.5, normalize=False)
    got["reverberate noise only, positional"] = run(ops.reverberate, f32, [800, 1], dry, 1 << 64, 3, 0.0, 1.0, 1)
    got["reverberate Nmax 0"] = run(ops.reverberate, torch.zeros(2, 0), [0, 0], bank, 5)
    return got


def _cmvn_cases(run):
    got = {}
    x = _feats()
    B, T, F = x.shape
    one = lambda: torch.zeros(2, F + 1, dtype=torch.float64)                       # noqa: E731
    per = lambda G: torch.ones(G, 2, F + 1, dtype=torch.float64)                   # noqa: E731
    got["cmvn_accumulate"] = run(ops.cmvn_accumulate, x, torch.tensor([9, 0]), one())
    got["cmvn_accumulate Tmax 0"] = run(ops.cmvn_accumulate, torch.zeros(2, 0, F), torch.tensor([0, 0]), one())
    got["cmvn_accumulate_groups host ids, host frames"] = run(ops.cmvn_accumulate_groups, x, [9, 0], [2, 0], per(3))
    got["cmvn_accumulate_groups tensor ids, tensor frames"] = run(ops.cmvn_accumulate_groups, x, torch.tensor([4, 9]), torch.tensor([1, 1]), per(2))
    got["cmvn_accumulate_groups Tmax 0"] = run(ops.cmvn_accumulate_groups, torch.zeros(2, 0, F), [0, 0], [0, 0], per(1))
    got["cmvn_apply one matrix, no groups"] = run(ops.cmvn_apply, x, [9, 0], one())
    got["cmvn_apply groups, means only, out"] = run(ops.cmvn_apply, x, torch.tensor([4, 9]), per(3), groups=[2, 1], norm_vars=False,
                                                    out=torch.empty(B, T, F))
    got["cmvn_apply in place"] = run(ops.cmvn_apply, x, [9, 9], per(1), out=x)
    got["cmvn_apply Tmax 0"] = run(ops.cmvn_apply, torch.zeros(2, 0, F), [0, 0], per(1), groups=[0, 0])
    got["cmvn_sliding defaults, host frames"] = run(ops.cmvn_sliding, x, [9, 0])
    got["cmvn_sliding options, tensor frames, out"] = run(ops.cmvn_sliding, x, torch.tensor([4, 9]), cmn_window=7, min_cmn_window=3,
                                                          normalize_variance=True, center=True, out=torch.empty(B, T, F))
    got["cmvn_sliding positional options"] = run(ops.cmvn_sliding, x, [9, 9], 5, 5, 1, 0)
    got["cmvn_sliding Tmax 0"] = run(ops.cmvn_sliding, torch.zeros(2, 0, F), [0, 0])
    out = torch.empty(B, T, F)
    got["cmvn_apply returns out itself"] = run(lambda: ops.cmvn_apply(x, [9, 9], per(1), out=out) is out)
    got["cmvn_sliding returns out itself"] = run(lambda: ops.cmvn_sliding(x, [9, 9], out=out) is out)
    return got


def _pitch_cases(run):
    got = {}
    f32, lens = _waves("float32", lens=(1400, 0), nmax=1600)
    i16, _ = _waves("int16", lens=(1400, 0), nmax=1600)
    plan = ops.PitchPlan()
    other = ops.PitchPlan(min_f0=60.0, max_f0=350.0, frame_length=20.0, frame_shift=5.0, upsample_filter_width=3, nccf_ballast=1000.0)
    got["pitch float32, host lengths"] = run(ops.pitch, f32, lens, plan)
    got["pitch int16, tensor lengths, lags, other plan"] = run(ops.pitch, i16, torch.tensor(lens), other, return_lags=True)
    got["pitch Tmax 0"] = run(ops.pitch, f32, [300, 0], plan)
    got["pitch Tmax 0, lags"] = run(ops.pitch, f32, [0, 0], plan, True)
    raw = torch.from_numpy(np.abs(np.random.RandomState(6).standard_normal((2, 9, 2))).astype(np.float32) + 60.0)
    got["pitch_process defaults, host frames"] = run(ops.pitch_process, raw, [9, 0])
    got["pitch_process options, tensor frames"] = run(
        ops.pitch_process, raw, torch.tensor([4, 9]), seed=-5, utt_offset=6, pitch_scale=1.5, pov_scale=0.5, pov_offset=0.25,
        delta_pitch_scale=5.0, delta_pitch_noise_stddev=0.0, normalization_left_context=10, normalization_right_context=20, delta_window=3,
        add_pov_feature=False, add_raw_log_pitch=True)
    got["pitch_process one column"] = run(ops.pitch_process, raw, [9, 9], 1 << 64, add_pov_feature=False, add_delta_pitch=False)
    got["pitch_process Tmax 0"] = run(ops.pitch_process, torch.zeros(2, 0, 2), [0, 0])
    return got


def test_device_entry_arguments_are_those_recorded_at_the_parent(run):
    got = {}
    for cases in (_features_cases, _resample_cases, _context_cases, _reverb_cases, _cmvn_cases, _pitch_cases):
        got.update(cases(run))
    got = json.loads(json.dumps(got))                                   # (tuples as lists, as the file holds them)
    seen = {c["entry"] for case in got.values() for c in case["calls"] if "entry" in c}
    assert seen == set(DEVICE_ENTRIES)
    if os.environ.get(RECORD):
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        pytest.fail("recorded %d cases into %s: unset %s to compare" % (len(got), GOLDEN, RECORD))
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name


def test_ops_and_frontend_hold_the_same_objects():
    from ctc_pytorch_amd import frontend
    for name in PUBLIC:
        assert getattr(ops, name) is getattr(frontend, name), name
    assert "ctc_pytorch_amd.ops" not in (frontend.fbank.__module__, frontend.FbankPlan.__module__)
