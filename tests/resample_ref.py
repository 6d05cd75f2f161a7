"""numpy restatement of the resampler (include/ctcn.h, ctcn_resample: Kaldi's LinearResample as ResampleWaveform configures it): the plan in
double, the output count, and the ascending float64 sum over float32 weights and float32 samples, rounded once.  Nothing here calls the
library."""
import math

import numpy as np

PAIRS = [(14400, 16000), (17600, 16000), (8000, 16000), (48000, 16000), (44100, 16000), (16000, 8000), (11025, 16000)]


def default_cutoff(fin, fout):
    return 0.99 * 0.5 * min(fin, fout)


def units(fin, fout):
    g = math.gcd(fin, fout)
    return fin // g, fout // g                                          # (iu, ou)


def num_samples(n, fin, fout):
    return 0 if n <= 0 else -((-n * fout) // fin)


def half_width(fin, fout, num_zeros=6, cutoff=None):
    cutoff = default_cutoff(fin, fout) if cutoff is None else cutoff
    return num_zeros / (2 * cutoff)


def plan(fin, fout, num_zeros=6, cutoff=None):
    """(first (ou) int, ntaps (ou) int, weights: list of ou float64 arrays, NOT rounded to float32)."""
    cutoff = default_cutoff(fin, fout) if cutoff is None else cutoff
    ww = num_zeros / (2 * cutoff)
    _, ou = units(fin, fout)
    first, ntaps, weights = [], [], []
    for i in range(ou):
        t_out = i / fout
        lo = math.ceil((t_out - ww) * fin)
        hi = math.floor((t_out + ww) * fin)
        w = np.zeros(hi - lo + 1, dtype=np.float64)
        for j in range(hi - lo + 1):
            dt = (lo + j) / fin - t_out
            win = 0.5 * (1 + math.cos(2 * math.pi * cutoff / num_zeros * dt)) if abs(dt) < ww else 0.0
            filt = math.sin(2 * math.pi * cutoff * dt) / (math.pi * dt) if dt != 0 else 2 * cutoff
            w[j] = filt * win / fin
        first.append(lo)
        ntaps.append(hi - lo + 1)
        weights.append(w)
    return np.asarray(first, dtype=np.int64), np.asarray(ntaps, dtype=np.int64), weights


def weight_table(fin, fout, num_zeros=6, cutoff=None):
    """plan()'s weights as the kernel stores them: (ou, longest tap count) float32, zeros behind a row's taps."""
    first, ntaps, weights = plan(fin, fout, num_zeros, cutoff)
    table = np.zeros((len(weights), int(ntaps.max())), dtype=np.float32)
    for i, w in enumerate(weights):
        table[i, :w.shape[0]] = w.astype(np.float32)
    return first, ntaps, table


def resample(x, fin, fout, first, ntaps, weights):
    """y (ceil(n fout / fin)) float32 of one utterance x (int16 or float32) on a weight table (ou, >= max ntaps) float32: for every output the
    sum over j ascending of float64(w[p][j]) * float64(x[first[p] + u iu + j]), samples outside [0, n) counting as zero, rounded once."""
    x = np.asarray(x)
    n = x.shape[0]
    iu, ou = units(fin, fout)
    m = num_samples(n, fin, fout)
    if m == 0:
        return np.zeros(0, dtype=np.float32)
    xs = x.astype(np.float32).astype(np.float64)
    w64 = np.asarray(weights, dtype=np.float32).astype(np.float64)
    k = np.arange(m, dtype=np.int64)
    u, p = k // ou, k % ou
    start = np.asarray(first, dtype=np.int64)[p] + u * iu
    nt = np.asarray(ntaps, dtype=np.int64)[p]
    acc = np.zeros(m, dtype=np.float64)
    for j in range(int(nt.max())):
        s = start + j
        ok = (j < nt) & (s >= 0) & (s < n)
        v = np.where(ok, xs[np.clip(s, 0, n - 1)], 0.0)
        acc = np.where(j < nt, acc + w64[p, j] * v, acc)
    return acc.astype(np.float32)


def two_tone(n, fin, fout, amplitude=1000.0):
    """The two-tone probe: tones of `amplitude` at 0.05 and 0.3 of the cutoff.  Returns (x (n) float32 at fin, y (ceil(n fout / fin)) float64:
    the same analytic signal at fout)."""
    cutoff = default_cutoff(fin, fout)
    f1, f2 = 0.05 * cutoff, 0.3 * cutoff
    sig = lambda t: amplitude * (np.sin(2 * np.pi * f1 * t) + np.sin(2 * np.pi * f2 * t + 0.7))
    return sig(np.arange(n) / fin).astype(np.float32), sig(np.arange(num_samples(n, fin, fout)) / fout)
