"""numpy restatement of Kaldi's MFCC computation (feature-mfcc on top of feature-window, feature-fbank's mel stage and ComputeDctMatrix), the
yardstick of tests/test_mfcc*.py.  Everything up to the log-mel energies and the log energy is tests/fbank_ref.py with use_power and
use_log_fbank; this file adds the DCT, the lifter, the energy rule and the HTK column order.  Kaldi's binaries are not available here:
equality with them is argued from this restatement of their documented algorithm, it has not been run.

`dtype` selects the arithmetic of the whole per-frame chain, as in fbank_ref.  The DCT table and the lifter are computed in float64 and
rounded once to `dtype` -- the plan builder of the library does the same."""
import numpy as np

import fbank_ref as R

DEFAULTS = dict(sample_frequency=16000.0, frame_shift=10.0, frame_length=25.0, dither=1.0, preemphasis_coefficient=0.97,
                remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, blackman_coeff=0.42, snip_edges=True,
                num_mel_bins=23, low_freq=20.0, high_freq=0.0, num_ceps=13, use_energy=True, energy_floor=0.0, raw_energy=True,
                cepstral_lifter=22.0, htk_compat=False)
_OWN = ("num_ceps", "cepstral_lifter")


def options(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def fbank_options(o):
    """The filterbank configuration whose log-mel energies (and energy column) the MFCC of `o` is taken from."""
    return R.options(use_power=True, use_log_fbank=True, **{k: v for k, v in o.items() if k not in _OWN})


def dct_matrix(num_bins, num_ceps):
    """float64 (C, N): the first C rows of Kaldi's ComputeDctMatrix."""
    n = np.arange(num_bins, dtype=np.float64)[None, :]
    k = np.arange(num_ceps, dtype=np.float64)[:, None]
    D = np.sqrt(2.0 / num_bins) * np.cos(np.pi / num_bins * (n + 0.5) * k)
    D[0, :] = np.sqrt(1.0 / num_bins)
    return D


def lifter(num_ceps, Q):
    """float64 (C): 1 + Q / 2 sin(pi k / Q); ones for Q = 0 (no lifter)."""
    if Q == 0:
        return np.ones(num_ceps)
    return 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(num_ceps, dtype=np.float64) / Q)


def htk_order(x):
    """Columns in HTK's order: the first one last, the others down by one."""
    return np.concatenate([x[..., 1:], x[..., :1]], axis=-1)


def cepstra(logmel, log_energy, o, dtype=np.float64):
    """Steps 2-5 on (T, N) log-mel rows and the (T) log energies (already floored; None without use_energy), in `dtype`: (T, C)."""
    N, C = o["num_mel_bins"], o["num_ceps"]
    assert logmel.shape[1] == N and logmel.dtype == dtype
    c = logmel @ dct_matrix(N, C).astype(dtype).T
    c = c * lifter(C, float(np.float32(o["cepstral_lifter"]))).astype(dtype)[None, :]
    assert c.dtype == dtype
    if o["use_energy"]:
        c[:, 0] = log_energy
    if o["htk_compat"]:
        if not o["use_energy"]:
            c[:, 0] = (c[:, 0].astype(np.float64) * np.sqrt(2.0)).astype(dtype)       # Kaldi's `*= M_SQRT2`: a double product, rounded once
        c = htk_order(c)
    return c


def split_fbank(fb, o):
    """(log-mel (T, N), log energy (T) or None) of a filterbank matrix computed with fbank_options(o)."""
    nb = o["num_mel_bins"]
    if not o["use_energy"]:
        return fb, None
    if o["htk_compat"]:
        return fb[:, :nb], fb[:, nb]
    return fb[:, 1:], fb[:, 0]


def mfcc(wave, o, dtype=np.float64):
    """(T, C) MFCCs of one 1-D waveform (Kaldi's scale), dither off, every per-frame operation in `dtype`."""
    fb = R.fbank(wave, fbank_options(o), dtype)
    m, e = split_fbank(fb, o)
    return cepstra(np.ascontiguousarray(m), e, o, dtype)
