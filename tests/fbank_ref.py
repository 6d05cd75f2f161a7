"""numpy restatement of Kaldi's filterbank computation (feature-window, feature-fbank, mel-computations) and of its global CMVN, the
yardstick of tests/test_fbank*.py.  Kaldi's binaries are not available here: equality with them is argued from this restatement of
their documented algorithm, it has not been run.

`dtype` selects the arithmetic of the whole per-frame chain: float64, or float32 with scipy.fft.rfft (which stays in single precision).
The window and the mel weights are computed in float64 and rounded once to `dtype` -- the plan builder of the library does the same -- so
the difference between the two dtypes is the arithmetic on the signal, not a second set of tables."""
import numpy as np
import scipy.fft

DEFAULTS = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, dither=1.0, preemphasis_coefficient=0.97,
                remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True,
                num_mel_bins=23, low_freq=20.0, high_freq=0.0, use_energy=False, energy_floor=0.0, raw_energy=True, htk_compat=False,
                use_log_fbank=True, use_power=True)
EPS = float(np.finfo(np.float32).eps)                                  # Kaldi's floor: std::numeric_limits<float>::epsilon()


def options(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def geometry(o):
    """(frame length, frame shift, padded length) in samples."""
    L = int(np.float32(o["sample_frequency"]) * 0.001 * np.float32(o["frame_length"]))
    shift = int(np.float32(o["sample_frequency"]) * 0.001 * np.float32(o["frame_shift"]))
    npad = 1 << (L - 1).bit_length() if o["round_to_power_of_two"] else L
    return L, shift, npad


def num_frames(n, L, shift, snip_edges):
    if snip_edges:
        return 0 if n < L else 1 + (n - L) // shift
    return (n + shift // 2) // shift


def feat_dim(o):
    return o["num_mel_bins"] + (1 if o["use_energy"] else 0)


def window(o):
    """float64 window of feature-window.cc."""
    L = geometry(o)[0]
    a = 2.0 * np.pi / (L - 1)
    i = np.arange(L, dtype=np.float64)
    kind = o["window_type"]
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(a * i)
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(a * i)
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(a * i)) ** 0.85
    if kind == "rectangular":
        return np.ones(L)
    if kind == "blackman":
        c = float(np.float32(o["blackman_coeff"]))
        return c - 0.5 * np.cos(a * i) + (0.5 - c) * np.cos(2 * a * i)
    raise ValueError(kind)


def mel(f):
    return 1127.0 * np.log(1.0 + f / 700.0)


def mel_bank(o):
    """[(first FFT bin, float64 weights)] per filter: mel-computations.cc without VTLN; FFT bins 0 .. npad/2 - 1."""
    npad = geometry(o)[2]
    sf = float(o["sample_frequency"])
    nyquist = 0.5 * sf
    low = float(o["low_freq"])
    high = float(o["high_freq"]) if o["high_freq"] > 0 else nyquist + float(o["high_freq"])
    nb = o["num_mel_bins"]
    mel_low, mel_high = mel(low), mel(high)
    delta = (mel_high - mel_low) / (nb + 1)
    mels = mel(sf / npad * np.arange(npad // 2, dtype=np.float64))
    bank = []
    for b in range(nb):
        left, center, right = mel_low + b * delta, mel_low + (b + 1) * delta, mel_low + (b + 2) * delta
        inside = np.nonzero((mels > left) & (mels < right))[0]
        assert inside.size and np.array_equal(inside, np.arange(inside[0], inside[-1] + 1))
        m = mels[inside]
        w = np.where(m <= center, (m - left) / (center - left), (right - m) / (right - center))
        if o["htk_compat"] and b == 0 and low != 0.0:
            w[0] = 0.0
        bank.append((int(inside[0]), w))
    return bank


def fbank(wave, o, dtype=np.float64):
    """(T, F) features of one 1-D waveform (Kaldi's scale), dither off, every per-frame operation in `dtype`."""
    assert dtype in (np.float64, np.float32)
    L, shift, npad = geometry(o)
    wave = np.asarray(wave)
    n = wave.shape[0]
    T = num_frames(n, L, shift, o["snip_edges"])
    F, nb = feat_dim(o), o["num_mel_bins"]
    if T == 0:
        return np.zeros((0, F), dtype=dtype)
    idx = np.arange(T)[:, None] * shift + np.arange(L)[None, :]
    if not o["snip_edges"]:
        idx += shift // 2 - L // 2
        while True:                                                    # Kaldi's reflection, repeated for signals shorter than the overhang
            bad = (idx < 0) | (idx >= n)
            if not bad.any():
                break
            idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))
    x = wave.astype(dtype)[idx]
    if o["remove_dc_offset"]:
        x = x - (x.sum(axis=1, dtype=dtype) / dtype(L))[:, None]
    energy = None
    if o["use_energy"] and o["raw_energy"]:
        energy = (x * x).sum(axis=1, dtype=dtype)
    c = dtype(np.float32(o["preemphasis_coefficient"]))
    if c != 0:
        x = x - c * np.concatenate([x[:, :1], x[:, :-1]], axis=1)
    x = x * window(o).astype(dtype)[None, :]
    if o["use_energy"] and not o["raw_energy"]:
        energy = (x * x).sum(axis=1, dtype=dtype)
    spec = scipy.fft.rfft(np.pad(x, ((0, 0), (0, npad - L))), axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    power = (spec.real * spec.real + spec.imag * spec.imag)[:, :npad // 2]
    if not o["use_power"]:
        power = np.sqrt(power)
    W = np.zeros((npad // 2, nb), dtype=dtype)
    for b, (first, w) in enumerate(mel_bank(o)):
        W[first:first + w.size, b] = w.astype(dtype)
    melE = power @ W
    assert melE.dtype == dtype
    if o["use_log_fbank"]:
        melE = np.log(np.maximum(melE, dtype(EPS)))
    out = np.empty((T, F), dtype=dtype)
    off = 1 if (o["use_energy"] and not o["htk_compat"]) else 0
    out[:, off:off + nb] = melE
    if o["use_energy"]:
        le = np.log(np.maximum(energy, dtype(EPS)))
        if o["energy_floor"] > 0:
            le = np.maximum(le, np.log(dtype(np.float32(o["energy_floor"]))))
        out[:, nb if o["htk_compat"] else 0] = le
    return out


def cmvn_stats(mats):
    """Kaldi's (2, F + 1) float64 statistics of a list of (T, F) matrices."""
    F = mats[0].shape[1]
    s = np.zeros((2, F + 1))
    for m in mats:
        m = m.astype(np.float64)
        s[0, :F] += m.sum(axis=0)
        s[1, :F] += (m * m).sum(axis=0)
        s[0, F] += m.shape[0]
    return s


def mean_scale(stats):
    """apply-cmvn --norm-vars=true: mean and 1 / sqrt(var) with var floored at 1e-20, in double, rounded once to float32."""
    stats = np.asarray(stats, dtype=np.float64)
    n = stats[0, -1]
    mean = stats[0, :-1] / n
    var = np.maximum(stats[1, :-1] / n - mean * mean, 1e-20)
    return mean.astype(np.float32), (1.0 / np.sqrt(var)).astype(np.float32)
