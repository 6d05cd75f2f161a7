"""The resampler's host side, without a GPU: the output count, the plan against the numpy restatement of tests/resample_ref.py, the host twin
ctcn_resample_host (the kernel's sum, the same plan block) bit for bit against the restatement on the plan's own weights, the two-tone probe
against its analytic form, the refusals, the allow_downsample / allow_upsample configuration keys and make_feat.py's key and label rewriting.

Weights: the C library's and numpy's sin / cos may differ in the last place, so a weight is held to the float32 rounding of the
restatement's double or the float32 next to it; the test prints how many differ (measured: DESIGN.md section 7l)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.steps import make_feat  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

PAIRS = RR.PAIRS
_PLANS, _REFS = {}, {}


def plan_of(pair):
    if pair not in _PLANS:
        _PLANS[pair] = ops.ResamplePlan(*pair)
    return _PLANS[pair]


def ref_of(pair):
    if pair not in _REFS:
        _REFS[pair] = RR.plan(*pair)
    return _REFS[pair]


def signal_lengths(pair, plan):
    """The signal lengths both suites use: 0, 1, 2; around half a filter (ceil(ww fin) - 1, itself, + 1); whole units (iu, 3 iu, 3 iu + 1: the
    last-sample rule); one sample before, on and after the input position of the kernel's first tile boundary; about two and a half tiles."""
    fin, fout = pair
    iu, ou = RR.units(fin, fout)
    half = int(np.ceil(RR.half_width(fin, fout) * fin))
    edge = plan.tile // ou * iu
    return [0, 1, 2, half - 1, half, half + 1, iu, 3 * iu, 3 * iu + 1, edge - 1, edge, edge + 1, (5 * edge) // 2 + 7]


def host_resample(plan, x):
    x = np.ascontiguousarray(x)
    m = RR.num_samples(x.shape[0], plan.orig_freq, plan.new_freq)
    out = np.full(m + 3, -12345.0, dtype=np.float32)
    r = _lib.lib().ctcn_resample_host(x.ctypes.data_as(ctypes.c_void_p), int(x.dtype == np.int16), x.shape[0], ctypes.byref(plan.opts),
                                      plan.host.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), m + 3)
    assert r == m, (r, m, _lib.lib().ctcn_last_error())
    assert np.all(out[m:] == -12345.0)
    return out[:m]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_sample_count(pair):
    fin, fout = pair
    iu, _ = RR.units(fin, fout)
    for n in range(4 * iu + 4):
        want = -((-n * fout) // fin)
        assert _lib.lib().ctcn_resample_samples(n, fin, fout) == want == ops.resample_samples(n, fin, fout) == RR.num_samples(n, fin, fout), n
    assert _lib.lib().ctcn_resample_samples(-1, fin, fout) == -1
    with pytest.raises(ValueError):
        ops.resample_samples(-1, fin, fout)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_plan_against_restatement(pair):
    fin, fout = pair
    plan = plan_of(pair)
    first, ntaps, weights = ref_of(pair)
    iu, ou = RR.units(fin, fout)
    assert (plan.iu, plan.ou) == (iu, ou) and plan.tile % ou == 0 and plan.tile >= ou
    assert plan.stride % 2 == 1 and plan.stride >= plan.max_taps == int(ntaps.max())
    assert np.array_equal(plan.first, first) and np.array_equal(plan.ntaps, ntaps)
    differ = total = 0
    sums = []
    for i, w in enumerate(weights):
        got = plan.weights[i]
        want = w.astype(np.float32)
        nt = w.shape[0]
        assert np.all(got[nt:] == 0.0)
        exact = got[:nt] == want
        near = (got[:nt] == np.nextafter(want, np.float32(np.inf))) | (got[:nt] == np.nextafter(want, np.float32(-np.inf)))
        assert np.all(exact | near), (i, got[:nt], want)
        differ += int((~exact).sum())
        total += nt
        sums.append(float(got[:nt].astype(np.float64).sum()))
    print("resample %d -> %d: %d phases, %d..%d taps, %d of %d weights differ from numpy's in the last place, phase sums %.5f..%.5f"
          % (fin, fout, ou, ntaps.min(), ntaps.max(), differ, total, min(sums), max(sums)))
    assert max(abs(s - 1.0) for s in sums) <= 2e-3


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_host_twin_is_the_restatement_bit_for_bit(pair):
    plan = plan_of(pair)
    rs = np.random.RandomState(pair[0] % 1000 + 3)
    for n in signal_lengths(pair, plan):
        x = rs.randint(-32768, 32768, size=n).astype(np.int16)
        want = RR.resample(x, pair[0], pair[1], plan.first, plan.ntaps, plan.weights)
        got = host_resample(plan, x)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (pair, n)
        assert np.array_equal(host_resample(plan, x.astype(np.float32)).view(np.uint32), want.view(np.uint32)), (pair, n)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_two_tones_against_the_analytic_signal(pair):
    fin, fout = pair
    plan = plan_of(pair)
    n = int(0.25 * fin)
    x, y = RR.two_tone(n, fin, fout)
    got = host_resample(plan, x).astype(np.float64)
    ww = RR.half_width(fin, fout)
    t = np.arange(y.shape[0]) / fout
    inside = (t >= ww) & (t <= (n - 1) / fin - ww)
    err = np.abs(got - y)[inside].max() / 1000.0
    print("resample %d -> %d: two tones, interior error %.3g of the amplitude over %d samples" % (fin, fout, err, int(inside.sum())))
    assert inside.sum() > 1000 and err <= 2e-3


def test_refusals():
    L = _lib.lib()
    cases = [dict(orig_freq=0, new_freq=16000), dict(orig_freq=16000, new_freq=-1), dict(orig_freq=16000, new_freq=8000, num_zeros=0),
             dict(orig_freq=16000, new_freq=8000, cutoff=4000.5),           # 2 cutoff > min(rates)
             dict(orig_freq=16000, new_freq=15999),                         # 15 999 phases of 13 taps: no LDS holds that table
             dict(orig_freq=16001, new_freq=16000)]
    for kw in cases:
        with pytest.raises(RuntimeError, match="rc=-3"):
            ops.ResamplePlan(**kw)
        opts = _lib.ResampleOpts(cutoff=kw.get("cutoff", 0.99 * 0.5 * min(kw["orig_freq"], kw["new_freq"])), orig_freq=kw["orig_freq"],
                                 new_freq=kw["new_freq"], num_zeros=kw.get("num_zeros", 6))
        assert L.ctcn_resample_plan_bytes(ctypes.byref(opts)) == 0
        buf = np.zeros(16, dtype=np.uint32)
        # the launch refuses the same options before it looks at anything else (no device is touched)
        assert L.ctcn_resample(None, 0, None, ctypes.byref(opts), None, None, 1, 0, 0, None) == -3
        assert L.ctcn_resample_host(None, 0, 0, ctypes.byref(opts), buf.ctypes.data_as(ctypes.c_void_p), None, 0) == -3
    assert L.ctcn_resample_samples(2 ** 31 - 1, 8000, 16000) == -3            # an output length beyond int32
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.resample_samples(2 ** 31 - 1, 8000, 16000)
    # what the budget must admit: 16 384 table floats -- 44.1 / 22.05 / 11.025 kHz to 16 and 8 kHz, every 0.01 speed factor at 16 kHz
    for fin in (44100, 22050, 11025):
        for fout in (16000, 8000):
            p = ops.ResamplePlan(fin, fout)
            assert p.ou * p.stride <= 16384
    for c in range(50, 201):
        if c != 100:
            p = ops.ResamplePlan(160 * c, 16000)
            assert p.ou <= 100
    # a plan of other options is not taken by the host twin
    a, b = plan_of((8000, 16000)), plan_of((48000, 16000))
    out = np.zeros(8, dtype=np.float32)
    x = np.zeros(4, dtype=np.int16)
    assert L.ctcn_resample_host(x.ctypes.data_as(ctypes.c_void_p), 1, 4, ctypes.byref(a.opts), b.host.ctypes.data_as(ctypes.c_void_p),
                                out.ctypes.data_as(ctypes.c_void_p), 8) == -1


def test_allow_options_parse_in_the_three_kaldi_configs(tmp_path):
    conf = tmp_path / "x.conf"
    for cls in (features.FbankConfig, features.MfccConfig, features.SpectrogramConfig):
        d = cls()
        assert d.allow_downsample is False and d.allow_upsample is False
        conf.write_text("--allow-downsample=true\n--dither=0\n")
        c = cls.from_kaldi_conf(str(conf))
        assert c.allow_downsample is True and c.allow_upsample is False and c.dither == 0.0
        conf.write_text("--allow-upsample   # a bare flag\n")
        c = cls.from_kaldi_conf(str(conf))
        assert c.allow_downsample is False and c.allow_upsample is True
        assert cls(allow_upsample=True, allow_downsample=True).allow_downsample is True
        c.c_opts()                                                          # the C struct has no such fields and is built all the same
        conf.write_text("--allow-upsample=maybe\n")
        with pytest.raises(ValueError):
            cls.from_kaldi_conf(str(conf))
    conf.write_text("--allow-downsample=true\n")
    with pytest.raises(ValueError, match="allow-downsample"):
        features.LogSpecConfig.from_kaldi_conf(str(conf))
    with pytest.raises(ValueError):
        features.LogSpecConfig(allow_upsample=True)


def test_rate_check_names_the_option():
    cfg = features.FbankConfig()
    assert make_feat.source_rate("u", "u.wav", 16000, cfg) == 16000
    with pytest.raises(ValueError, match="no resampling here.*allow-downsample"):
        make_feat.source_rate("u", "u.wav", 44100, cfg)
    with pytest.raises(ValueError, match="no resampling here.*allow-upsample"):
        make_feat.source_rate("u", "u.wav", 8000, cfg)
    with pytest.raises(ValueError, match="allow-upsample"):
        make_feat.source_rate("u", "u.wav", 8000, features.FbankConfig(allow_downsample=True))
    assert make_feat.source_rate("u", "u.wav", 8000, features.MfccConfig(allow_upsample=True)) == 8000
    assert make_feat.source_rate("u", "u.wav", 44100, features.SpectrogramConfig(allow_downsample=True)) == 44100
    with pytest.raises(ValueError, match=r"\(no resampling here\)"):
        make_feat.source_rate("u", "u.wav", 8000, features.LogSpecConfig())


def test_speed_perturb_keys_and_labels():
    f = make_feat.parse_factors("0.9,1.0,1.1")
    assert f == [("0.9", 0.9), ("1.0", 1.0), ("1.1", 1.1)]
    assert make_feat.parse_factors(" 1.10 , 1 ") == [("1.10", 1.1), ("1", 1.0)]
    for bad in ("", "0.9,,1.1", "0.9,-1", "fast", "0", "0.9,0.9", "nan", "inf"):
        with pytest.raises(ValueError):
            make_feat.parse_factors(bad)
    assert make_feat.perturbed_keys(["a", "b"], None) == ["a", "b"]
    assert make_feat.perturbed_keys(["a", "b"], f) == ["sp0.9-a", "sp1.0-a", "sp1.1-a", "sp0.9-b", "sp1.0-b", "sp1.1-b"]
    lines = ["spk_utt0 sil hh ax l ow sil\n", "\n", "spk_utt1 sil\n", "spk_utt2\n", "spk_utt3   b  iy"]
    got = make_feat.perturb_text(lines, make_feat.parse_factors("1.1,0.9"))
    assert got == ["sp1.1-spk_utt0 sil hh ax l ow sil\n", "sp0.9-spk_utt0 sil hh ax l ow sil\n", "sp1.1-spk_utt1 sil\n", "sp0.9-spk_utt1 sil\n",
                   "sp1.1-spk_utt2\n", "sp0.9-spk_utt2\n", "sp1.1-spk_utt3 b  iy\n", "sp0.9-spk_utt3 b  iy\n"]
    with pytest.raises(ValueError, match="speed-perturb"):
        make_feat.main(["--conf", "x", "--wav-scp", "y", "--out-dir", "z", "--text", "t"])


def test_speed_perturb_rates():
    """Perturbing by f reads round(rate f) -> rate: 0.9 and 1.1 at 16 kHz are the pairs 14400 -> 16000 and 17600 -> 16000."""
    assert [int(round(16000 * f)) for _, f in make_feat.parse_factors("0.9,1.0,1.1")] == [14400, 16000, 17600]
    n = 16000
    assert ops.resample_samples(n, 14400, 16000) == int(np.ceil(n / 0.9)) and ops.resample_samples(n, 17600, 16000) == int(np.ceil(n / 1.1))
