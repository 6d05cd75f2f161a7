"""Reverberation and additive noise without a GPU: ctcn_reverb_bank, ctcn_reverb_plan and ctcn_reverb_host (the draw, gain, mix and scale code
the kernels are compiled from) against the numpy restatement of the contract (tests/reverb_ref.py), bit for bit; checks that do not go
through the restatement (a shifted impulse, the unit impulse, np.convolve with the bound of one float32 rounding plus the worst float64
accumulation error, the output power under normalisation, the measured SNR); the refusals; steps/make_feat.py's keys and labels.
CASES is shared with tests/test_reverb.py, which holds the kernels to the same numbers."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_ref as RV  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.steps import make_feat  # noqa: E402

TILE, TAP_CHUNK, POW_CHUNK, MAX_TAPS = 2048, 1024, 1024, 16384      # pinned here; test_limits_are_the_pinned_ones holds them to the library
SNRS = (20.0, 10.0, 0.0, -5.0)
_BUILT = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rir(K, peak, seed):
    """K taps of decaying noise with the largest value at `peak`."""
    rs = np.random.RandomState(seed)
    h = (rs.randn(K) * np.exp(-np.arange(K) / max(K / 4.0, 1.0)) * 0.3).astype(np.float32)
    h[peak] = np.float32(1.0) + np.abs(h).max()
    return h


def noise(L, seed, scale=300.0):
    return (np.random.RandomState(seed).randn(L) * scale).astype(np.float32)


# name -> (impulse responses, noises, sample frequency, utterance lengths, int16 input).  fs = 1000: the early window is [p - 1, p + 50).
CASES = {
    # n at tile - 1, tile, tile + 1, 0, 1; the early tail (33 taps) of 1020 crosses a power chunk, that of tile - 1 a tile as well
    "tile_edges": ([rir(37, 5, 1)], [noise(1500, 2)], 1000, [TILE - 1, TILE, TILE + 1, 0, 1, 1020], True),
    "tile_edges_f32": ([rir(37, 5, 1)], [noise(1500, 2)], 1000, [TILE - 1, TILE, TILE + 1, 0, 1, 1020], False),
    # K at chunk - 1 with the peak at 0 (lo clamps); a noise of 7 samples wraps hundreds of times; n < K
    "chunk_minus_1": ([rir(TAP_CHUNK - 1, 0, 3)], [noise(7, 4)], 1000, [700, TILE + 500], True),
    # K at chunk with the peak at K - 1 (hi clamps); a noise longer than any utterance
    "chunk": ([rir(TAP_CHUNK, TAP_CHUNK - 1, 5)], [noise(5000, 6)], 1000, [1500, TILE + 1000], False),
    # K at chunk + 1; an all-zero noise row: skipped
    "chunk_plus_1": ([rir(TAP_CHUNK + 1, 400, 7)], [np.zeros(50, dtype=np.float32)], 1000, [1030, TILE + 2], True),
    # more than two tap chunks, n < K and n > K, 16 kHz windows (16 before, 800 behind the peak)
    "three_chunks": ([rir(2100, 30, 8)], [noise(333, 9)], 16000, [300, 2300, TILE + 300], False),
    # the longest impulse response the call takes: all sixteen tap chunks walked, n < K; the early window is 16 + 800 taps
    "max_taps": ([rir(MAX_TAPS, 5000, 17)], [noise(41, 18)], 16000, [300, TILE + 52], True),
    # several rows to draw from, a ragged batch
    "banks": ([rir(37, 5, 10), rir(600, 100, 11), rir(1, 0, 12)], [noise(7, 13), np.zeros(9, dtype=np.float32), noise(4100, 14)], 16000,
              [4100, 17, 0, 2049, 1, 999, TILE], True),
    # rows around a tap chunk that end well inside the row stride: what lies behind them must never be read
    "ragged_banks": ([rir(TAP_CHUNK + 1, 400, 19), rir(TAP_CHUNK - 1, 0, 20), rir(90, 20, 21)],
                     [np.zeros(50, dtype=np.float32), noise(1500, 22), noise(7, 23)], 1000, [1030, TILE + 2, 700, 5, TILE - 1, 1500, 64, 900], False),
    # one bank empty
    "no_noise": ([rir(90, 20, 15)], [], 1000, [1100, 5], True),
    "no_rir": ([], [noise(100, 16)], 1000, [2100, 64], False),
}
SEED = 20240607


def built(name):
    """(ops.ReverbBank, RV.Bank, the padded batch, lengths), once per case."""
    if name not in _BUILT:
        rirs, noises, fs, lens, i16 = CASES[name]
        rs = np.random.RandomState(len(name) * 131 + 7)
        batch = np.zeros((len(lens), max(lens)), dtype=np.int16 if i16 else np.float32)
        for b, n in enumerate(lens):
            batch[b, :n] = rs.randint(-20000, 20001, size=n) if i16 else (rs.randn(n) * 3000.0).astype(np.float32)
        _BUILT[name] = (ops.ReverbBank(rirs, noises, fs, SNRS), RV.Bank(rirs, noises, fs, SNRS), batch, lens)
    return _BUILT[name]


_WANT = {}


def want(name, **kw):
    """The restatement's output of every utterance of a case (utterance b is number 3 + b of the stream), computed once."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _WANT:
        _, ref, batch, lens = built(name)
        _WANT[key] = [RV.reverberate(batch[b, :n], ref, SEED, 3 + b, **kw) for b, n in enumerate(lens)]
    return _WANT[key]


def test_limits_are_the_pinned_ones():
    lim = ops.reverb_limits()
    assert (lim["tile"], lim["tap_chunk"], lim["power_chunk"], lim["max_taps"], lim["max_snrs"]) == (TILE, TAP_CHUNK, POW_CHUNK, MAX_TAPS, 16)
    assert RV.CHUNK == lim["power_chunk"] and lim["tile"] % lim["power_chunk"] == 0 and lim["run"] * 256 == lim["tile"]
    assert lim["max_taps"] >= 16384


@pytest.mark.parametrize("name", sorted(CASES))
def test_bank_quantities_are_the_restatement(name):
    bank, ref, _, _ = built(name)
    assert bank.R == len(ref.rirs) and bank.N == len(ref.noises)
    assert [tuple(int(v) for v in row) for row in bank.rir_meta] == ref.meta
    assert [int(v) for v in bank.noise_len] == [q.shape[0] for q in ref.noises]
    assert np.array_equal(np.asarray(bank.noise_power).view(np.uint64), np.asarray(ref.noise_power, dtype=np.float64).view(np.uint64))
    assert np.array_equal(np.asarray(bank.snr_gain).view(np.uint64), np.asarray(ref.snr_gain, dtype=np.float64).view(np.uint64))
    for r, (K, p, lo, hi) in enumerate(ref.meta):
        assert 0 <= lo <= p < hi <= K
    if name == "chunk_minus_1":
        assert ref.meta[0][1:3] == (0, 0)                               # lo clamped
    if name == "chunk":
        assert ref.meta[0][1] == TAP_CHUNK - 1 and ref.meta[0][3] == TAP_CHUNK   # hi clamped


def test_bank_block_ignores_what_lies_behind_a_row():
    """NaN behind every row's length in the caller's padded rows: the block is the one built from the bare rows."""
    rirs, noises, fs, _, _ = CASES["banks"]
    bank = built("banks")[0]
    L = _lib.lib()
    h = np.full((len(rirs), 700), np.nan, dtype=np.float32)
    q = np.full((len(noises), 4200), np.nan, dtype=np.float32)
    for i, r in enumerate(rirs):
        h[i, :r.shape[0]] = r
    for i, r in enumerate(noises):
        q[i, :r.shape[0]] = r
    hl, ql = np.asarray([r.shape[0] for r in rirs], dtype=np.int32), np.asarray([r.shape[0] for r in noises], dtype=np.int32)
    snrs = np.asarray(SNRS, dtype=np.float64)
    nbytes = L.ctcn_reverb_bank_bytes(3, 700, 3, 4200, 4)
    buf = np.zeros(nbytes // 4, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    assert L.ctcn_reverb_bank(p(h), p(hl), 3, 700, p(q), p(ql), 3, 4200, p(snrs), 4, float(fs), p(buf), nbytes) == 0
    assert not np.isnan(buf.view(np.float32)[buf.view(np.int32)[11]:]).any()
    x = built("banks")[2][0]
    o = _lib.ReverbOpts(rir_prob=1.0, noise_prob=1.0, normalize=1)
    for u in range(6):
        out = np.zeros(x.shape[0], dtype=np.float32)
        assert L.ctcn_reverb_host(p(x), 1, x.shape[0], p(buf), ctypes.byref(o), SEED, u, p(out)) == 0
        assert np.array_equal(bits(out), bits(ops.reverberate_host(x, bank, SEED, u)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_is_the_restatement(name):
    bank, ref, _, _ = built(name)
    seen = set()
    for seed in (0, 1, SEED, (1 << 64) - 1):
        for u in (0, 1, 2, 255, 256, (1 << 56) - 1):
            for probs in ((1.0, 1.0), (0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.3, 0.9)):
                got = ops.reverb_plan(bank, seed, u, *probs)
                assert got == RV.plan(ref, seed, u, *probs), (seed, u, probs)
                seen.add((got["rir"] is None, got["noise"] is None))
                if got["noise"] is not None:
                    assert 0 <= got["offset"] < ref.noises[got["noise"]].shape[0] and 0 <= got["snr"] < len(SNRS)
    if bank.R and bank.N:
        assert len(seen) == 4                                           # every combination of on and off was drawn


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_is_the_restatement_bit_for_bit(name, normalize):
    bank, _, batch, lens = built(name)
    for b, n in enumerate(lens):
        got = ops.reverberate_host(batch[b, :n], bank, SEED, 3 + b, normalize=normalize)
        w = want(name, normalize=normalize)[b]
        assert got.shape == w.shape == (n,) and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(w)), (name, b, n, int((bits(got) != bits(w)).sum()))
        assert np.isfinite(got).all()


def test_host_twin_with_drawn_probabilities():
    bank, ref, batch, lens = built("banks")
    kinds = set()
    for u in range(24):
        x = batch[u % len(lens), :lens[u % len(lens)]]
        pl = RV.plan(ref, 77, u, 0.5, 0.6)
        kinds.add((pl["rir"], pl["noise"]))
        assert np.array_equal(bits(ops.reverberate_host(x, bank, 77, u, rir_prob=0.5, noise_prob=0.6)), bits(RV.reverberate(x, ref, 77, u, 0.5, 0.6)))
    assert len(kinds) >= 6


def near_end_seed(bank, u, L, slack=1):
    """A seed under which utterance u draws a noise offset within `slack` of the row's last sample."""
    for seed in range(4000):
        pl = ops.reverb_plan(bank, seed, u)
        if pl["offset"] is not None and pl["offset"] >= L - 1 - slack:
            return seed
    raise AssertionError("no seed with an offset near %d" % (L - 1))


def test_noise_wraps_from_an_offset_near_its_end():
    bank, ref, batch, lens = built("chunk_minus_1")
    seed = near_end_seed(bank, 0, 7, slack=0)
    assert ops.reverb_plan(bank, seed, 0)["offset"] == 6
    x = batch[1, :lens[1]]
    st = RV.stages(x, ref, seed, 0, normalize=False)
    assert np.array_equal(bits(ops.reverberate_host(x, bank, seed, 0, normalize=False)), bits(st["out"]))
    q = ref.noises[0].astype(np.float64)
    assert np.array_equal(st["added"][:9], st["g"] * q[[6, 0, 1, 2, 3, 4, 5, 6, 0]])


# ---- checks that do not go through the restatement ----------------------------------------------------------------------------------------

def signal(n, seed, i16=False):
    rs = np.random.RandomState(seed)
    return rs.randint(-20000, 20001, size=n).astype(np.int16) if i16 else (rs.randn(n) * 2000.0 + 1.0).astype(np.float32)


@pytest.mark.parametrize("k0,K", [(0, 1), (1, 2), (5, 9), (1023, 1024), (1024, 1030), (1500, 2100)])
def test_a_shifted_impulse_shifts_the_signal(k0, K):
    h = np.zeros(K, dtype=np.float32)
    h[k0] = 1.0
    bank = ops.ReverbBank([h], [noise(10, 1)], 16000, SNRS)
    for n in (1, 700, 2049, TILE + 1):
        x = signal(n, n + k0)
        y = ops.reverberate_host(x, bank, 1, 0, noise_prob=0.0, normalize=False)
        shifted = np.zeros(n, dtype=np.float32)
        shifted[k0:] = x[:max(n - k0, 0)]
        assert np.array_equal(bits(y), bits(shifted)), (k0, K, n)


def test_the_unit_impulse_and_both_parts_off_keep_the_input_bits():
    one = ops.ReverbBank([np.ones(1, dtype=np.float32)], [], 16000)
    for n, i16 in ((1, False), (2049, False), (3000, True)):
        x = signal(n, 5 + n, i16)
        for normalize in (True, False):
            assert np.array_equal(bits(ops.reverberate_host(x, one, 9, 4, normalize=normalize)), bits(x.astype(np.float32)))
    bank = built("banks")[0]
    x = signal(2500, 3)
    x[7] = -0.0
    for normalize in (True, False):
        assert np.array_equal(bits(ops.reverberate_host(x, bank, 9, 4, rir_prob=0.0, noise_prob=0.0, normalize=normalize)), bits(x))


@pytest.mark.parametrize("name", ["tile_edges_f32", "chunk", "three_chunks"])
def test_convolution_against_numpy_convolve(name):
    """|y - c| <= 2^-24 |c| + K 2^-53 sum |h||x| element by element: one float32 rounding plus the worst case of K float64 additions."""
    bank, ref, batch, lens = built(name)
    h = ref.rirs[0].astype(np.float64)
    K = h.shape[0]
    for b, n in enumerate(lens):
        if n == 0:
            continue
        x = batch[b, :n].astype(np.float64)
        y = ops.reverberate_host(batch[b, :n], bank, SEED, 3 + b, noise_prob=0.0, normalize=False).astype(np.float64)
        c = np.convolve(x, h)[:n]
        bound = 2.0 ** -24 * np.abs(c) + K * 2.0 ** -53 * np.convolve(np.abs(x), np.abs(h))[:n]
        worst = float(np.max(np.abs(y - c) - bound))
        print("%s n %d: max |y - c| %.3g, max of |y - c| - bound %.3g" % (name, n, float(np.abs(y - c).max()), worst))
        assert worst <= 0.0, (name, n, worst)


@pytest.mark.parametrize("name", ["tile_edges", "chunk", "banks", "no_rir"])
def test_normalised_output_has_the_input_power(name):
    """out[i] = fl32(s z[i]) with s^2 S(z) = S(x): the power differs from the input's by one float32 rounding of every sample, a factor
    within (1 +- 2^-24)^2, plus the float64 rounding of the sums and of s (2^-40 covers them at these lengths)."""
    bank, _, batch, lens = built(name)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        x = batch[b, :n].astype(np.float64)
        out = ops.reverberate_host(batch[b, :n], bank, SEED, 3 + b).astype(np.float64)
        ratio = math.fsum(out * out) / math.fsum(x * x)
        print("%s n %d: output power / input power - 1 = %.3g" % (name, n, ratio - 1.0))
        assert abs(ratio - 1.0) <= (1 + 2.0 ** -24) ** 2 - 1 + 2.0 ** -40, (name, b, ratio - 1.0)


@pytest.mark.parametrize("with_rir", [False, True])
def test_measured_snr_is_the_drawn_one(with_rir):
    """The noise row is an exact divisor of the utterance, so the added term has the row's power.  d = z - y differs from the float64 term by
    at most half an ulp of z per sample, so rms(d) lies within 2^-24 rms(z) of the term's; 2^-30 covers the float64 roundings."""
    L, n, fs = 7, 7 * 300, 1000
    h = rir(60, 10, 21)
    q = noise(L, 22)
    bank = ops.ReverbBank([h] if with_rir else [], [q], fs, SNRS)
    x = signal(n, 23)
    for u in range(8):
        pl = ops.reverb_plan(bank, 31, u)
        y = ops.reverberate_host(x, bank, 31, u, noise_prob=0.0, normalize=False).astype(np.float64)
        z = ops.reverberate_host(x, bank, 31, u, normalize=False).astype(np.float64)
        d = z - y
        if with_rir:
            e = np.convolve(x.astype(np.float64), h.astype(np.float64)[9:60])        # [p - 1, min(K, p + 50))
            e = e.astype(np.float32).astype(np.float64)
        else:
            e = x.astype(np.float64)
        p_sig, p_add = math.fsum(e * e) / e.shape[0], math.fsum(d * d) / n
        measured = 10.0 * math.log10(p_sig / p_add)
        rel = 2.0 ** -24 * math.sqrt(math.fsum(z * z) / n) / math.sqrt(p_add) + 2.0 ** -30
        tol = 20.0 * math.log10(1.0 + rel) * 1.0001
        print("u %d: drawn %g dB, measured - drawn %.3g dB (tolerance %.3g)" % (u, SNRS[pl["snr"]], measured - SNRS[pl["snr"]], tol))
        assert abs(measured - SNRS[pl["snr"]]) <= tol


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    h, q = [np.ones(4, dtype=np.float32)], [np.ones(5, dtype=np.float32)]
    with pytest.raises(RuntimeError, match="taps"):
        ops.ReverbBank([np.zeros(0, dtype=np.float32)], q, 16000)
    with pytest.raises(RuntimeError, match="samples"):
        ops.ReverbBank(h, [np.zeros(0, dtype=np.float32)], 16000)
    with pytest.raises(RuntimeError, match="16 384") as e:
        ops.ReverbBank([np.ones(MAX_TAPS + 1, dtype=np.float32)], q, 16000)
    assert "rc=-3" in str(e.value)
    ops.ReverbBank([np.ones(MAX_TAPS, dtype=np.float32)], q, 16000)
    with pytest.raises(RuntimeError, match="16 SNRs") as e:
        ops.ReverbBank(h, q, 16000, snrs=range(17))
    assert "rc=-3" in str(e.value)
    ops.ReverbBank(h, q, 16000, snrs=range(16))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="not finite"):
            ops.ReverbBank(h, q, 16000, snrs=[10, bad])
        with pytest.raises(RuntimeError, match="not finite"):
            ops.ReverbBank([np.asarray([1.0, bad], dtype=np.float32)], q, 16000)
    with pytest.raises(RuntimeError, match="empty"):
        ops.ReverbBank([], [], 16000)
    with pytest.raises(RuntimeError, match="SNR"):
        ops.ReverbBank(h, q, 16000, snrs=[])
    with pytest.raises(RuntimeError, match="sample_frequency"):
        ops.ReverbBank(h, q, 0)
    bank = ops.ReverbBank(h, q, 16000)
    x = np.ones(8, dtype=np.float32)
    for kw in (dict(rir_prob=-0.1), dict(rir_prob=1.5), dict(noise_prob=float("nan")), dict(noise_prob=2.0)):
        with pytest.raises(RuntimeError, match="probability"):
            ops.reverberate_host(x, bank, 1, 0, **kw)
        with pytest.raises(RuntimeError, match="probability"):
            ops.reverb_plan(bank, 1, 0, **kw)
    with pytest.raises(TypeError):
        ops.reverberate_host(x, "bank", 1, 0)
    # the device call refuses before any launch: no device is touched
    L = _lib.lib()
    keep = (ctypes.create_string_buffer(64), ctypes.create_string_buffer(64))
    fake, other = (ctypes.c_void_p(ctypes.addressof(k)) for k in keep)
    for o in (_lib.ReverbOpts(rir_prob=2.0, noise_prob=0.0, normalize=1), _lib.ReverbOpts(rir_prob=0.0, noise_prob=-1.0, normalize=1)):
        assert L.ctcn_reverb(fake, 0, fake, bank._host_ptr(), fake, ctypes.byref(o), 1, 0, other, 1, 8, fake, 1 << 20, None) == -1
    ok = _lib.ReverbOpts(rir_prob=1.0, noise_prob=1.0, normalize=1)
    assert L.ctcn_reverb(fake, 0, fake, fake, fake, ctypes.byref(ok), 1, 0, other, 1, 8, fake, 1 << 20, None) == -1          # not a bank block
    assert L.ctcn_reverb(fake, 0, fake, bank._host_ptr(), fake, ctypes.byref(ok), 1, 0, fake, 1, 8, fake, 1 << 20, None) == -1   # out aliases wave
    assert L.ctcn_reverb(fake, 0, fake, bank._host_ptr(), fake, ctypes.byref(ok), 1, 0, other, 0, 8, fake, 1 << 20, None) == -1  # B
    assert L.ctcn_reverb(fake, 0, fake, bank._host_ptr(), fake, ctypes.byref(ok), 1, 0, other, 1, 8, fake, 8, None) == -4        # workspace
    assert L.ctcn_reverb_ws_bytes(bank._host_ptr(), 1, 8) >= 8 * (4 + 8) and L.ctcn_reverb_ws_bytes(bank._host_ptr(), 0, 8) == 0


def test_empty_utterance_and_shapes():
    bank = built("banks")[0]
    assert ops.reverberate_host(np.zeros(0, dtype=np.float32), bank, 1, 0).shape == (0,)
    with pytest.raises(ValueError):
        ops.reverberate_host(np.zeros((2, 3), dtype=np.float32), bank, 1, 0)
    silent = ops.reverberate_host(np.zeros(100, dtype=np.int16), bank, 1, 0)
    assert np.isfinite(silent).all()                                   # P_in = 0: g = 0 or s = 0, never 0 / 0


# ---- steps/make_feat.py ---------------------------------------------------------------------------------------------------------------------

def write_wav(path, samples, rate=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples, dtype="<i2").tobytes())


def test_make_feat_keys_labels_and_lists(tmp_path):
    assert make_feat.reverb_keys(["a", "b"], 0) == ["a", "b"]
    assert make_feat.reverb_keys(["a", "b"], 2) == ["a", "rev1-a", "rev2-a", "b", "rev1-b", "rev2-b"]
    sp = make_feat.perturbed_keys(["u"], make_feat.parse_factors("0.9,1.0"))
    assert make_feat.reverb_keys(sp, 1) == ["sp0.9-u", "rev1-sp0.9-u", "sp1.0-u", "rev1-sp1.0-u"]
    lines = ["u1 a b c\n", "\n", "u2 d\n"]
    assert make_feat.rewrite_text(lines, None, 1) == ["u1 a b c\n", "rev1-u1 a b c\n", "u2 d\n", "rev1-u2 d\n"]
    assert make_feat.rewrite_text(lines, make_feat.parse_factors("1.1"), 2) == [
        "sp1.1-u1 a b c\n", "rev1-sp1.1-u1 a b c\n", "rev2-sp1.1-u1 a b c\n", "sp1.1-u2 d\n", "rev1-sp1.1-u2 d\n", "rev2-sp1.1-u2 d\n"]
    assert make_feat.rewrite_text(lines, make_feat.parse_factors("1.1,0.9"), 0) == make_feat.perturb_text(lines, make_feat.parse_factors("1.1,0.9"))
    assert make_feat.parse_snrs("20,15, 10,5,0") == [20.0, 15.0, 10.0, 5.0, 0.0]
    for bad in ("", "a", "1,,2", "nan", "inf", ",".join(["1"] * 17)):
        with pytest.raises(ValueError):
            make_feat.parse_snrs(bad)
    # list files: one path per line (or `<name> <path>`), read by read_wave; the same rate passes through without a device
    h = (rir(40, 3, 1) * 8000).astype(np.int16)
    write_wav(tmp_path / "h.wav", h)
    write_wav(tmp_path / "q.wav", np.arange(50))
    (tmp_path / "rirs.txt").write_text("%s\n\n" % (tmp_path / "h.wav"))
    (tmp_path / "noises.txt").write_text("babble %s\n" % (tmp_path / "q.wav"))
    rows = make_feat.read_wave_list(str(tmp_path / "rirs.txt"), 16000, "cpu", 1 << 20)
    assert len(rows) == 1 and np.array_equal(rows[0], h)
    rows = make_feat.read_wave_list(str(tmp_path / "noises.txt"), 16000, "cpu", 1 << 20)
    assert len(rows) == 1 and np.array_equal(rows[0], np.arange(50))
    (tmp_path / "none.txt").write_text("\n")
    with pytest.raises(ValueError, match="no waves"):
        make_feat.read_wave_list(str(tmp_path / "none.txt"), 16000, "cpu", 1 << 20)


def test_make_feat_refuses_inconsistent_reverb_options():
    common = ["--conf", "x", "--wav-scp", "y", "--out-dir", "z"]
    for bad in (["--reverb-copies", "1"], ["--rir-list", "r"], ["--noise-list", "n", "--reverb-copies", "0"], ["--rir-list", "r", "--reverb-copies", "-1"],
                ["--rir-list", "r", "--reverb-copies", "1", "--rir-prob", "1.5"], ["--rir-list", "r", "--reverb-copies", "1", "--noise-prob", "-0.5"],
                ["--noise-list", "n", "--reverb-copies", "1", "--snrs", "1,x"], ["--snrs", "1,2"], ["--rir-prob", "0.5"], ["--reverb-seed", "3"]):
        with pytest.raises(ValueError):
            make_feat.main(common + bad)
    with pytest.raises(ValueError, match="--speed-perturb or --reverb-copies"):
        make_feat.main(common + ["--text", "t"])
