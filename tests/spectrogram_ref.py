"""numpy restatements of the two spectrogram front-ends, the yardsticks of tests/test_spectrogram*.py.

spectrogram   Kaldi's compute-spectrogram-feats (feature-spectrogram over feature-window): tests/fbank_ref.py's geometry, frame count and
              window, its per-frame chain up to the transform, then the log power of bins 0 .. Npad / 2 and the log energy in column 0.
log_spectrum  the recipe's timit/local/make_spectrum.py as numpy states it: np.pad(y, n_fft // 2, "reflect"), strided frames,
              scipy.signal.windows.<name>(n_fft, sym=True), rfft, abs, log1p, (m - m.mean()) / m.std().

Neither Kaldi nor librosa / torchaudio is available here: equality with them is argued from these restatements of their documented
algorithms, it has not been run.  `dtype` selects the arithmetic of the whole chain: float64, or float32 with scipy.fft.rfft (which stays
in single precision).  Window tables are formed in float64 and rounded once to `dtype`, as the library's plan builders do."""
import numpy as np
import scipy.fft
import scipy.signal.windows

import fbank_ref as R

EPS = R.EPS
KALDI_DEFAULTS = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, dither=1.0, preemphasis_coefficient=0.97,
                      remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True,
                      energy_floor=0.0, raw_energy=True, return_raw_fft=False)
STFT_DEFAULTS = dict(sample_rate=16000.0, window_size=0.025, window_stride=0.01, window="hamming", normalize=True, input_scale=1.0)


def options(**kw):
    unknown = set(kw) - set(KALDI_DEFAULTS)
    assert not unknown, unknown
    return dict(KALDI_DEFAULTS, **kw)


def stft_options(**kw):
    unknown = set(kw) - set(STFT_DEFAULTS)
    assert not unknown, unknown
    return dict(STFT_DEFAULTS, **kw)


def fbank_options(o, **kw):
    """The filterbank options of fbank_ref that share the frame options of a spectrogram configuration (energy on: column 0)."""
    keep = {k: v for k, v in o.items() if k in R.DEFAULTS}
    return R.options(**dict(keep, use_energy=True, **kw))


def feat_dim(o):
    return R.geometry(fbank_options(o))[2] // 2 + 1


def spectrogram(wave, o, dtype=np.float64):
    """(T, Npad / 2 + 1) features of one 1-D waveform (Kaldi's scale), dither off, every per-frame operation in `dtype`."""
    assert dtype in (np.float64, np.float32) and not o["return_raw_fft"]
    fo = fbank_options(o)
    L, shift, npad = R.geometry(fo)
    wave = np.asarray(wave)
    n = wave.shape[0]
    T = R.num_frames(n, L, shift, o["snip_edges"])
    F = npad // 2 + 1
    if T == 0:
        return np.zeros((0, F), dtype=dtype)
    idx = np.arange(T)[:, None] * shift + np.arange(L)[None, :]
    if not o["snip_edges"]:
        idx += shift // 2 - L // 2
        while True:                                                    # Kaldi's reflection (the edge sample IS repeated), as fbank_ref
            bad = (idx < 0) | (idx >= n)
            if not bad.any():
                break
            idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))
    x = wave.astype(dtype)[idx]
    if o["remove_dc_offset"]:
        x = x - (x.sum(axis=1, dtype=dtype) / dtype(L))[:, None]
    if o["raw_energy"]:
        energy = (x * x).sum(axis=1, dtype=dtype)
    c = dtype(np.float32(o["preemphasis_coefficient"]))
    if c != 0:
        x = x - c * np.concatenate([x[:, :1], x[:, :-1]], axis=1)
    x = x * R.window(fo).astype(dtype)[None, :]
    if not o["raw_energy"]:
        energy = (x * x).sum(axis=1, dtype=dtype)
    spec = scipy.fft.rfft(np.pad(x, ((0, 0), (0, npad - L))), axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64) and spec.shape[1] == F
    out = np.log(np.maximum(spec.real * spec.real + spec.imag * spec.imag, dtype(EPS)))
    le = np.log(np.maximum(energy, dtype(EPS)))
    if o["energy_floor"] > 0:
        le = np.maximum(le, np.log(dtype(np.float32(o["energy_floor"]))))
    out[:, 0] = le
    assert out.dtype == dtype
    return out


def stft_geometry(o):
    """(n_fft, hop) in samples: the reference's int(sample_rate * window_size), int(sample_rate * window_stride)."""
    return int(o["sample_rate"] * o["window_size"]), int(o["sample_rate"] * o["window_stride"])


def stft_num_frames(n, hop):
    return 0 if n == 0 else 1 + n // hop


def stft_window(o):
    """float64, scipy's symmetric form: what librosa gets when it calls the reference's scipy.signal.<name> with the window length."""
    return getattr(scipy.signal.windows, o["window"])(stft_geometry(o)[0], sym=True)


def stft_frames(y, n_fft, hop):
    """The centred frames of librosa.stft: (1 + n // hop, n_fft) over the reflected signal."""
    p = np.pad(y, n_fft // 2, mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(p, n_fft)[::hop]


def log_spectrum(wave, o, dtype=np.float64):
    """(raw (T, n_fft / 2 + 1), normalised, (mean, std)) of one 1-D waveform; mean and std (ddof = 0) over all values, in `dtype`."""
    assert dtype in (np.float64, np.float32)
    n_fft, hop = stft_geometry(o)
    F = n_fft // 2 + 1
    y = (np.asarray(wave).astype(np.float32) * np.float32(o["input_scale"])).astype(dtype)      # input_scale: a float32 product, first
    if y.shape[0] == 0:
        return np.zeros((0, F), dtype=dtype), np.zeros((0, F), dtype=dtype), (dtype(0), dtype(0))
    x = stft_frames(y, n_fft, hop) * stft_window(o).astype(dtype)[None, :]
    spec = scipy.fft.rfft(x, axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64) and spec.shape == (stft_num_frames(y.shape[0], hop), F)
    raw = np.log1p(np.abs(spec))
    m, s = raw.mean(), raw.std()
    with np.errstate(invalid="ignore", divide="ignore"):
        normed = np.divide(np.add(raw, -m), s)
    assert raw.dtype == dtype and normed.dtype == dtype
    return raw, normed, (m, s)
