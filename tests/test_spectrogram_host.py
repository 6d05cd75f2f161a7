"""Host-side checks of the two spectrogram front-ends (no GPU): the transform's butterflies through ctcn_fbank_power_host (the kernels' own
passes and split step with a loop over the 64 lanes), the plan builders against the tables of tests/spectrogram_ref.py, the frame-count rule
of the STFT, the restatements themselves, the config readers and every refusal.

Bounds.  Transform: the issue's 1e-9 of the frame's energy per bin of the power spectrum (float64 passes leave ~1e-15 of it).  Window tables:
both sides evaluate one double expression (the Kaldi windows are then rounded once to float32, the STFT's stay double); scipy forms the cosine
sums over linspace(-pi, pi), the library over 2 pi i / (N - 1), so the doubles may differ by two ulps of 1 and a rounding by one float32 ulp.  Twiddles: one cos / sin each, 1 ulp of a
double at 1.  float32 restatement against the float64 one: the figures of the issue (section "The tolerance"), which the GPU tests measure
again as e32.
The issue lists -2 for an unknown window; -2 is CTCN_EHIP, the code of a HIP runtime error.  The plan builders answer a bad option value
with CTCN_EINVAL (-1) everywhere else (the filterbank's unknown window type among them), and so do these."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fbank_ref as R  # noqa: E402
import spectrogram_ref as SR  # noqa: E402
from test_mfcc import make_signals  # noqa: E402
from test_mfcc_host import ulps  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

SIGNALS = make_signals()
TONE = 2                                                                # the bare 1 kHz tone of make_signals


def power_host(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    p = np.full(x.size // 2 + 1, -1.0)
    assert _lib.lib().ctcn_fbank_power_host(x.ctypes.data_as(ctypes.c_void_p), x.size, p.ctypes.data_as(ctypes.c_void_p)) == 0
    return p


@pytest.mark.parametrize("n", [256, 400, 512, 1024])
def test_transform_against_a_direct_dft(n):
    k = np.arange(n // 2 + 1)
    dft = np.exp(-2j * np.pi * np.outer(k, np.arange(n)) / n)           # the definition, in float64
    rs = np.random.RandomState(n)
    frames = {"noise": 3000.0 * rs.standard_normal(n), "alternating": 1000.0 * (-1.0) ** np.arange(n), "constant": np.full(n, 1000.0)}
    for pos in (0, 1, 7, n // 2 - 1, n // 2, n - 1):
        frames["impulse at %d" % pos] = np.eye(n)[pos] * 1000.0
    worst = 0.0
    for name, x in frames.items():
        got, want = power_host(x), np.abs(dft @ x) ** 2
        err = float(np.abs(got - want).max() / (x * x).sum())
        worst = max(worst, err)
        assert err <= 1e-9, (n, name, err)
    assert abs(power_host(frames["alternating"])[n // 2] - (1000.0 * n) ** 2) <= 1e-9 * (1000.0 * n) ** 2      # the Nyquist bin: (Re Z0 - Im Z0)^2
    assert abs(power_host(frames["constant"])[0] - (1000.0 * n) ** 2) <= 1e-9 * (1000.0 * n) ** 2
    assert np.abs(power_host(frames["impulse at 7"]) - 1e6).max() <= 1e-3                                      # flat
    print("n = %d: largest |power - direct DFT| / frame energy = %.3g over %d frames" % (n, worst, len(frames)))


def test_transform_refuses_other_lengths():
    L = _lib.lib()
    x = np.zeros(320)
    assert L.ctcn_fbank_power_host(x.ctypes.data_as(ctypes.c_void_p), 320, x.ctypes.data_as(ctypes.c_void_p)) == -3
    assert L.ctcn_fbank_power_host(None, 400, x.ctypes.data_as(ctypes.c_void_p)) == -1


@pytest.mark.parametrize("kw,npad", [(dict(), 512), (dict(window_type="hamming"), 512), (dict(sample_frequency=8000.0), 256),
                                     (dict(frame_length=50.0, window_type="blackman"), 1024)])
def test_spectrogram_plan_is_the_head_of_the_filterbank_plan(kw, npad):
    cfg = features.SpectrogramConfig(**kw)
    plan = ops.SpectrogramPlan(cfg.c_opts())
    assert plan.padded_length == npad and plan.feat_dim == cfg.feat_dim == npad // 2 + 1 == SR.feat_dim(SR.options(**kw))
    assert plan.host.size == 5 * npad and _lib.lib().ctcn_spectrogram_plan_bytes(ctypes.byref(cfg.c_opts())) == 20 * npad
    fb = ops.FbankPlan(features.FbankConfig(**kw).c_opts())
    assert np.array_equal(plan.host, fb.host[:5 * npad])
    win = plan.host.view(np.float32)[:npad]
    L = plan.frame_length
    assert ulps(win[:L].copy(), R.window(SR.fbank_options(SR.options(**kw))).astype(np.float32)) <= 1 and not win[L:].any()
    tw = plan.host[npad:].view(np.float64).reshape(npad, 2)
    ang = 2.0 * np.pi * np.arange(npad) / npad
    assert np.abs(tw[:, 0] - np.cos(ang)).max() <= 2.3e-16 and np.abs(tw[:, 1] + np.sin(ang)).max() <= 2.3e-16


@pytest.mark.parametrize("window", features.LOGSPEC_WINDOWS)
@pytest.mark.parametrize("rate,size,n_fft", [(16000.0, 0.025, 400), (8000.0, 0.032, 256), (16000.0, 0.032, 512), (16000.0, 0.064, 1024)])
def test_logspec_plan_against_the_restatement(window, rate, size, n_fft):
    cfg = features.LogSpecConfig(sample_rate=rate, window_size=size, window=window)
    plan = ops.LogSpecPlan(cfg.c_opts())
    o = SR.stft_options(sample_rate=rate, window_size=size, window=window)
    assert (plan.n_fft, plan.hop) == SR.stft_geometry(o) == (cfg.n_fft, cfg.hop) == (n_fft, int(rate * 0.01))
    assert plan.feat_dim == cfg.feat_dim == n_fft // 2 + 1
    W = (n_fft + 63) // 64 * 64
    assert plan.host.size == 2 * W + 4 * n_fft and _lib.lib().ctcn_logspec_plan_bytes(ctypes.byref(cfg.c_opts())) == 4 * plan.host.size
    win = plan.host[:2 * W].view(np.float64)                           # kept in float64
    want = SR.stft_window(o)
    assert np.abs(win[:n_fft] - want).max() <= 4.5e-16 and ulps(win[:n_fft].astype(np.float32), want.astype(np.float32)) <= 1 and not win[n_fft:].any()
    assert win[0] == win[n_fft - 1]                                     # symmetric: a periodic window's last value is its second
    tw = plan.host[2 * W:].view(np.float64).reshape(n_fft, 2)
    ang = 2.0 * np.pi * np.arange(n_fft) / n_fft
    assert np.abs(tw[:, 0] - np.cos(ang)).max() <= 2.3e-16 and np.abs(tw[:, 1] + np.sin(ang)).max() <= 2.3e-16


def test_stft_frame_count_rule():
    L = _lib.lib()
    assert L.ctcn_logspec_frames(0, 160) == 0 and SR.stft_num_frames(0, 160) == 0
    assert L.ctcn_logspec_frames(-1, 160) == -1 and L.ctcn_logspec_frames(10, 0) == -1
    plan = ops.LogSpecPlan(features.LogSpecConfig().c_opts())
    for n in range(1, 1001):
        want = SR.stft_frames(np.zeros(n), 400, 160).shape[0]           # np.pad + striding, as librosa frames a centred signal
        assert L.ctcn_logspec_frames(n, 160) == want == 1 + n // 160 == plan.num_frames(n) == SR.stft_num_frames(n, 160), n
    for n in (1, 79, 80, 81, 255):
        assert L.ctcn_logspec_frames(n, 80) == SR.stft_frames(np.zeros(n), 256, 80).shape[0]


@pytest.mark.parametrize("n_fft", [256, 400, 512, 1024])
def test_stft_frames_per_workgroup_follow_the_lds_total(n_fft):
    """The STFT kernel's LDS total, seen through ctcn_logspec_ws_bytes (two doubles per workgroup, so its size shows the frames of one): 4-byte
    words of twiddles (4 n_fft), wave buffers (16 n_fft), partial sums (16), the float64 window (2 x n_fft rounded up to 64) and the samples
    of fpw frames ((fpw - 1) hop + n_fft); eight frames where that fits in 160 KB, else four, two, one -- at the very hop where the total
    crosses, for every length."""
    L = _lib.lib()
    fixed = 20 * n_fft + 16 + 2 * ((n_fft + 63) // 64 * 64) + n_fft
    limit = 160 * 1024 // 4

    def frames_per_workgroup(hop):
        o = features.LogSpecConfig().c_opts()
        o.window_size, o.window_stride = (n_fft + 0.5) / 16000.0, (hop + 0.5) / 16000.0
        assert ops.LogSpecPlan(o).n_fft == n_fft and ops.LogSpecPlan(o).hop == hop
        blocks = L.ctcn_logspec_ws_bytes(ctypes.byref(o), 1, 8) // 16
        assert blocks in (1, 2, 4, 8) and L.ctcn_logspec_ws_bytes(ctypes.byref(o), 3, 8) == 3 * 16 * blocks
        return 8 // blocks

    assert fixed < limit and frames_per_workgroup(1) == 8 and frames_per_workgroup(160) == 8 and frames_per_workgroup(999999) == 1
    for fpw in (8, 4, 2):
        last = (limit - fixed) // (fpw - 1)                               # the longest hop at which fpw frames' samples still fit
        assert fixed + (fpw - 1) * last <= limit < fixed + (fpw - 1) * (last + 1)
        assert (frames_per_workgroup(last), frames_per_workgroup(last + 1)) == (fpw, fpw // 2), (n_fft, fpw, last)


LDS_LAYOUT_CHECK = r"""
#include <stddef.h>
#include <stdio.h>
#include "fbank_core.h"
// the pointer arithmetic of the kernels and the size formulas of their launches before FbankLds / LogSpecLds (words of 4 bytes, a double is two)
template <int N> static bool fbank_is() {
  typedef FbankLds<N> T;
  return offsetof(T, tw) == 0 && offsetof(T, wbuf) == 4 * (2 * 2 * N) && offsetof(T, win) == offsetof(T, wbuf) + 4 * (2 * 8 * N) &&
         offsetof(T, wts) == offsetof(T, win) + 4 * N && offsetof(T, ftab) == offsetof(T, wts) + 4 * N &&
         sizeof(T) == offsetof(T, wts) + 4 * (N + 3 * FBANK_MAX_BINS) && sizeof(T) == 4 * (22 * N + 3 * FBANK_MAX_BINS) && fbank_lds_head(N) == sizeof(T);
}
template <int N> static bool logspec_is() {
  typedef LogSpecLds<N> T;
  const int wpad = (N + 63) / 64 * 64;
  return offsetof(T, tw) == 0 && offsetof(T, wbuf) == 4 * (2 * 2 * N) && offsetof(T, red) == offsetof(T, wbuf) + 4 * (2 * 8 * N) &&
         offsetof(T, win) == offsetof(T, red) + 8 * 8 && sizeof(T) == offsetof(T, win) + 8 * wpad && sizeof(T) == 4 * (20 * N + 16 + 2 * wpad) &&
         logspec_lds_head(N) == sizeof(T) && offsetof(T, red) % 8 == 0;
}
int main() {
  long n = 0, bad = 0;
  bad += !fbank_is<256>() + !fbank_is<512>() + !fbank_is<1024>() + !logspec_is<256>() + !logspec_is<400>() + !logspec_is<512>() + !logspec_is<1024>();
  const int npads[] = {256, 512, 1024}, nffts[] = {256, 400, 512, 1024}, fpws[] = {1, 2, 4, 8}, shifts[] = {1, 80, 160, 441, 3000, 999999};
  for (int npad : npads) for (int kind = KIND_FBANK; kind <= KIND_SPEC; ++kind) for (int fpw : fpws) for (int shift : shifts)
    for (int L = npad / 2 + 1; L <= npad; L += 37) for (int nbins = 3; nbins <= 128; nbins += 25) for (int F = 1; F <= (nbins < 64 ? nbins : 64); F += 9, ++n) {
      const size_t extra = kind == KIND_MFCC ? nbins * F + F : 0;         // the parent's fbank_lds_words(npad, L, shift, fpw, extra)
      bad += fbank_lds_head(npad) / 4 + fbank_lds_table(nbins, F, kind) + lds_samples(fpw, shift, L) != (size_t)22 * npad + 3 * FBANK_MAX_BINS + extra + (size_t)(fpw - 1) * shift + L;
    }
  for (int N : nffts) for (int fpw : fpws) for (int hop : shifts) {    // the parent's logspec_lds_words(nfft, wpad, hop, fpw)
    bad += logspec_lds_head(N) / 4 + lds_samples(fpw, hop, N) != (size_t)20 * N + 16 + 2 * ((N + 63) / 64 * 64) + (size_t)(fpw - 1) * hop + N;
    ++n;
  }
  printf("%ld layouts, %ld differ\n", n, bad);
  return bad != 0;
}
"""


def test_lds_layouts_are_the_kernels_earlier_pointer_arithmetic(tmp_path):
    """FbankLds and LogSpecLds of fbank_core.h (the structs the spectral kernels read their LDS through and their launches size it from),
    compiled for the host: every member's offset and the size for every length, and the total over Npad x kind x frames per workgroup x
    shift x L x bins x columns and N x frames x hop, equal the hand-written pointer arithmetic and size formulas they replaced -- a
    swapped pair of regions or a miscounted one shows here."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = shutil.which("g++") or shutil.which("c++") or os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = tmp_path / "lds_layout_check.cpp"
    src.write_text(LDS_LAYOUT_CHECK)
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-I", csrc, str(src), "-o", str(tmp_path / "check")], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = subprocess.run([str(tmp_path / "check")], capture_output=True, text=True)
    print(out.stdout.strip())
    assert out.returncode == 0 and " 0 differ" in out.stdout and int(out.stdout.split()[0]) > 60000, out.stdout + out.stderr


def test_reflection_of_the_restatement_by_hand():
    y = np.arange(5.0)                                                  # period 2 (n - 1) = 8, the edge sample not repeated, folded twice
    assert np.array_equal(np.pad(y, 9, mode="reflect"), [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3])
    assert np.array_equal(np.pad(np.array([7.0]), 3, mode="reflect"), [7.0] * 7)               # n = 1 is constant
    assert np.array_equal(np.pad(np.array([1.0, 2.0]), 3, mode="reflect"), [2, 1, 2, 1, 2, 1, 2, 1])


KALDI_CONFIGS = {"defaults": dict(), "hamming": dict(window_type="hamming"), "reflected_edges": dict(snip_edges=False),
                 "8khz": dict(sample_frequency=8000.0), "50ms": dict(frame_length=50.0)}
KALDI_E32 = {"defaults": 2.5e-4, "hamming": 4.7e-4, "reflected_edges": 8.8e-4, "8khz": 2.4e-4, "50ms": 7.1e-4}        # the issue's figures


@pytest.mark.parametrize("name", sorted(KALDI_CONFIGS))
def test_float32_restatement_follows_float64_kaldi(name):
    o = SR.options(dither=0.0, **KALDI_CONFIGS[name])
    worst = 0.0
    for i, s in enumerate(SIGNALS):
        r64, r32 = SR.spectrogram(s, o, np.float64), SR.spectrogram(s, o, np.float32)
        assert r64.shape == r32.shape == (R.num_frames(s.shape[0], *R.geometry(SR.fbank_options(o))[:2], o["snip_edges"]), SR.feat_dim(o))
        if not r64.size:
            continue
        e32 = float(np.abs(r32.astype(np.float64) - r64).max())
        if i == TONE and o["window_type"] == "povey":                   # its nulls sit at the FLT_EPSILON floor: the one case the rule leaves out
            print("%s: tone e32 %.3g (left out)" % (name, e32))
            continue
        worst = max(worst, e32)
    print("%s: largest e32 %.3g (the issue: %.3g)" % (name, worst, KALDI_E32[name]))
    assert 0.0 < worst <= 1.05 * KALDI_E32[name]                        # (the issue's figures carry two digits)


def test_float32_restatement_follows_float64_stft():
    o = SR.stft_options()
    raw_worst = norm_worst = 0.0
    for s in SIGNALS[1:]:
        (a64, b64, _), (a32, b32, _) = SR.log_spectrum(s, o, np.float64), SR.log_spectrum(s, o, np.float32)
        raw_worst = max(raw_worst, float(np.abs(a32.astype(np.float64) - a64).max()))
        norm_worst = max(norm_worst, float(np.abs(b32.astype(np.float64) - b64).max()))
    print("stft: largest e32 raw %.3g, normalised %.3g (the issue: 4.1e-4, 3.0e-4)" % (raw_worst, norm_worst))
    assert raw_worst <= 1.05 * 4.1e-4 and norm_worst <= 1.05 * 3.0e-4
    # what plausible mistakes move (the issue: 3.4 and 11): far beyond any bound the GPU tests use
    s = SIGNALS[4]
    raw = SR.log_spectrum(s, o)[0]
    periodic = np.log1p(np.abs(np.fft.rfft(SR.stft_frames(s.astype(np.float64), 400, 160) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(400) / 400)), axis=1)))
    edge = np.pad(s.astype(np.float64), 200, mode="symmetric")
    repeated = np.log1p(np.abs(np.fft.rfft(np.lib.stride_tricks.sliding_window_view(edge, 400)[::160] * SR.stft_window(o), axis=1)))
    d_edge = np.abs(repeated - raw).max(axis=1)
    print("periodic window moves %.3g, an edge-repeating reflection %.3g" % (np.abs(periodic - raw).max(), d_edge.max()))
    assert np.abs(periodic - raw).max() > 1.0 and d_edge[:2].max() > 1.0 and d_edge[2:-2].max() == 0.0


def test_restatements_by_hand():
    x = np.round(3000.0 * np.random.RandomState(1).standard_normal(4000))
    o = SR.options(dither=0.0)
    c = SR.spectrogram(x, o, np.float64)
    fb = R.fbank(x, SR.fbank_options(o), np.float64)
    assert c.shape == (23, 257) and np.array_equal(c[:, 0], fb[:, 0])   # column 0 is the filterbank's energy column
    # one bin from the definition: frame 5, bin 100 and the Nyquist bin
    L, shift, npad = 400, 160, 512
    fr = x[5 * shift:5 * shift + L]
    fr = fr - fr.mean()
    fr = (fr - float(np.float32(0.97)) * np.concatenate([fr[:1], fr[:-1]])) * R.window(SR.fbank_options(o))
    for k in (100, 256):
        X = (fr * np.exp(-2j * np.pi * k * np.arange(L) / npad)).sum()
        assert abs(c[5, k] - np.log(abs(X) ** 2)) <= 1e-9
    # energy after the window, and the floor
    assert not np.array_equal(SR.spectrogram(x, SR.options(dither=0.0, raw_energy=False))[:, 0], c[:, 0])
    fl = SR.spectrogram(x, SR.options(dither=0.0, energy_floor=3.6e9))
    assert (fl[:, 0] == np.log(np.float64(np.float32(3.6e9)))).any() and (fl[:, 0] > np.log(3.6e9)).any() and np.array_equal(fl[:, 1:], c[:, 1:])
    # the STFT: one value from the definition, frame 3 (samples 280 .. 680), bin 50; the statistics are over all values
    so = SR.stft_options()
    raw, normed, (m, s) = SR.log_spectrum(x, so)
    assert raw.shape == (26, 201)
    X = (x[280:680] * SR.stft_window(so) * np.exp(-2j * np.pi * 50 * np.arange(400) / 400)).sum()
    assert abs(raw[3, 50] - np.log1p(abs(X))) <= 1e-9
    assert abs(normed.mean()) <= 1e-12 and abs(normed.std() - 1.0) <= 1e-12 and m == raw.mean() and s == raw.std()
    scaled = SR.log_spectrum(x, SR.stft_options(input_scale=1.0 / 32768.0))[0]
    assert abs(scaled[3, 50] - np.log1p(abs(X) / 32768.0)) <= 1e-9


def test_config_readers(tmp_path):
    d = features.SpectrogramConfig.DEFAULTS
    assert d == SR.KALDI_DEFAULTS and "num_mel_bins" not in d and d["return_raw_fft"] is False
    assert features.LogSpecConfig.DEFAULTS == SR.STFT_DEFAULTS
    conf = tmp_path / "spectrogram.conf"
    conf.write_text("--window-type=hamming  # a comment\n--dither=0\n--energy-floor=1.5\n--raw-energy=false\n--return-raw-fft=false\n")
    c = features.SpectrogramConfig.from_kaldi_conf(str(conf))
    assert (c.window_type, c.dither, c.energy_floor, c.raw_energy, c.return_raw_fft, c.feat_dim) == ("hamming", 0.0, 1.5, False, False, 257)
    o = c.c_opts()
    assert (o.window_type, o.raw_energy, o.return_raw_fft, o.round_to_power_of_two, o.snip_edges, o.remove_dc_offset) == (0, 0, 0, 1, 1, 1)
    assert abs(o.energy_floor - 1.5) == 0 and abs(o.preemph_coeff - np.float32(0.97)) == 0
    conf.write_text("--return-raw-fft\n")                               # accepted by the reader, refused by the plan builder
    assert features.SpectrogramConfig.from_kaldi_conf(str(conf)).return_raw_fft is True
    conf.write_text("--num-mel-bins=40\n")
    with pytest.raises(ValueError, match="num-mel-bins"):
        features.SpectrogramConfig.from_kaldi_conf(str(conf))
    conf.write_text("--return-raw-fft=false\n")                         # a spectrogram key is no filterbank key
    with pytest.raises(ValueError, match="return-raw-fft"):
        features.FbankConfig.from_kaldi_conf(str(conf))
    conf.write_text("")                                                 # logspec: an empty file gives the recipe's audio_conf
    e = features.LogSpecConfig.from_kaldi_conf(str(conf))
    assert all(getattr(e, k) == v for k, v in SR.STFT_DEFAULTS.items()) and (e.n_fft, e.hop, e.feat_dim) == (400, 160, 201)
    conf.write_text("--sample-rate=8000\n--window-size=0.032\n--window=hann\n--normalize=false\n--input-scale=0.25\n")
    e = features.LogSpecConfig.from_kaldi_conf(str(conf))
    assert (e.sample_rate, e.n_fft, e.hop, e.window, e.normalize, e.input_scale) == (8000.0, 256, 80, "hann", False, 0.25)
    lo = e.c_opts()
    assert (lo.sample_rate, lo.window_size, lo.window_stride, lo.input_scale, lo.window, lo.normalize) == (8000.0, 0.032, 0.01, 0.25, 1, 0)
    conf.write_text("--dither=0\n")
    with pytest.raises(ValueError, match="dither"):
        features.LogSpecConfig.from_kaldi_conf(str(conf))
    with pytest.raises(ValueError, match="unknown window 'povey'"):
        features.LogSpecConfig(window="povey")


def test_refusals_come_from_the_plan_builders():
    L = _lib.lib()
    for kw, code in ((dict(return_raw_fft=True), -3), (dict(round_to_power_of_two=False), -3), (dict(frame_length=100.0), -3),
                     (dict(frame_length=5.0), -3), (dict(preemphasis_coefficient=1.5), -1)):
        cfg = features.SpectrogramConfig(**kw)
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            ops.SpectrogramPlan(cfg.c_opts())
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            features.Spectrogram(cfg, "cpu")
        assert L.ctcn_spectrogram_plan_bytes(ctypes.byref(cfg.c_opts())) == 0, kw
    bad = features.SpectrogramConfig().c_opts()
    bad.window_type = 9
    assert L.ctcn_spectrogram_plan(ctypes.byref(bad), None, 0) == -1 and L.ctcn_spectrogram_plan_bytes(ctypes.byref(bad)) == 0
    for kw, code in ((dict(window_size=0.02), -3), (dict(window_size=0.05), -3), (dict(sample_rate=0.0), -1), (dict(window_stride=0.00001), -1),
                     (dict(input_scale=0.0), -1)):
        cfg = features.LogSpecConfig(**kw)
        assert kw != dict(window_size=0.02) or cfg.n_fft == 320
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            ops.LogSpecPlan(cfg.c_opts())
        with pytest.raises(RuntimeError, match=r"rc=%d" % code):
            features.LogSpectrum(cfg, "cpu")
        assert L.ctcn_logspec_plan_bytes(ctypes.byref(cfg.c_opts())) == 0 and L.ctcn_logspec_ws_bytes(ctypes.byref(cfg.c_opts()), 4, 100) == 0
    lo = features.LogSpecConfig().c_opts()
    lo.window = 7                                                       # an unknown window (the config class raises ValueError before it gets here)
    assert L.ctcn_logspec_plan(ctypes.byref(lo), None, 0) == -1 and b"unknown window" in L.ctcn_last_error()
    ok = features.LogSpecConfig().c_opts()
    small = np.zeros(16, dtype=np.uint32)
    assert L.ctcn_logspec_plan(ctypes.byref(ok), small.ctypes.data_as(ctypes.c_void_p), small.nbytes) == -1 and not small.any()
    assert L.ctcn_logspec_plan(None, None, 0) == -1 and L.ctcn_logspec_plan_bytes(None) == 0 and L.ctcn_spectrogram_plan_bytes(None) == 0
    assert L.ctcn_logspec_ws_bytes(ctypes.byref(ok), 4, 100) == 4 * 13 * 16                     # one (sum, sum of squares) per eight frames
    # the filterbank and the MFCC keep their own refusal
    with pytest.raises(RuntimeError, match=r"rc=-3"):
        ops.FbankPlan(features.FbankConfig(round_to_power_of_two=False).c_opts())


def test_ops_raise_for_cpu_tensors_and_foreign_plans():
    sp = ops.SpectrogramPlan(features.SpectrogramConfig().c_opts())
    ls = ops.LogSpecPlan(features.LogSpecConfig().c_opts())
    fb = ops.FbankPlan(features.FbankConfig().c_opts())
    mf = ops.MfccPlan(features.MfccConfig().c_opts())
    x = torch.zeros(1, 400)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spectrogram(x, [400], sp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.log_spectrum(x, [400], ls)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        features.LogSpectrum(features.LogSpecConfig(), "cpu")([np.zeros(400, dtype=np.int16)])
    for plan in (fb, mf, ls):
        with pytest.raises(TypeError, match="SpectrogramPlan"):
            ops.spectrogram(x, [400], plan)
    for plan in (fb, mf, sp):
        with pytest.raises(TypeError, match="LogSpecPlan"):
            ops.log_spectrum(x, [400], plan)
    for plan in (sp, ls, mf):
        with pytest.raises(TypeError, match="FbankPlan"):
            ops.fbank(x, [400], plan)
    for plan in (sp, ls, fb):
        with pytest.raises(TypeError, match="MfccPlan"):
            ops.mfcc(x, [400], plan)
    with pytest.raises(ValueError, match=r"expected wave \(B, Nmax\)"):
        ops.log_spectrum(torch.zeros(400), [400], ls)


def test_make_feat_refuses_global_cmvn_for_logspec(tmp_path):
    from ctc_pytorch_amd.steps import make_feat
    (tmp_path / "logspec.conf").write_text("")
    (tmp_path / "wav.scp").write_text("")
    common = ["--feat-type", "logspec", "--conf", str(tmp_path / "logspec.conf"), "--wav-scp", str(tmp_path / "wav.scp"),
              "--out-dir", str(tmp_path / "out")]
    for extra in (["--compute-cmvn"], ["--cmvn-stats", str(tmp_path / "stats.txt")]):
        with pytest.raises(ValueError, match="per utterance|every utterance"):
            make_feat.main(common + extra)
    assert not (tmp_path / "out").exists()
    assert sorted(make_feat.FEAT_TYPES) == ["fbank", "logspec", "mfcc", "spectrogram"]
