"""Reverberation and additive noise as include/ctcn.h specifies them, restated in numpy on top of oracle.philox.philox4x32_10  --  TEST
INFRASTRUCTURE ONLY.

Written from the text of the contract, not from reverb.hip:

    S(v): float64 squares of the float32 elements, chunks of 1024 with zeros behind the last element, each chunk reduced by the halving
          tree t[j] += t[j + 512], + 256, ..., + 1, the chunk sums added in ascending order from 0
    rnd(word, n) = ((word >> 8) * n) >> 24; draw(d) = philox4(seed, (u << 8) | d)
    draw 0: on if R > 0 and rnd(w0, 2^24) < floor(float64(float32(rir_prob)) 2^24); r = rnd(w1, R)
    draw 1: on if N > 0 and rnd(w0, 2^24) < floor(float64(float32(noise_prob)) 2^24); m = rnd(w1, N), j = rnd(w2, J), off = rnd(w3, L_m)
    bank:   P_m = S(q_m) / L_m; p = first index of the largest tap; lo = max(0, p - floor(0.001 fs)), hi = min(K, p + floor(0.05 fs));
            G_j = 10 ** (-snr_j / 10) in float64
    P_in = S(x) / n; y = float32(ascending float64 sum of h[k] x[i - k]) for i < n; e = the same over h[lo:hi] and the full length
    n + (hi - lo) - 1; P_sig = S(e) / len(e) (without an RIR: y = x, P_sig = P_in)
    g = sqrt((G_j P_sig) / P_m); z = float32(float64(y) + g float64(q[(off + i) mod L]))   (numpy never fuses; P_m = 0: z = y)
    P_out = S(z) / n; > 0: out = float32(sqrt(P_in / P_out) float64(z)), else out = z."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.philox import philox4x32_10  # noqa: E402

U64 = (1 << 64) - 1
CHUNK = 1024


def power_sum(v):
    """S(v) of the contract; v float32."""
    v = np.asarray(v, dtype=np.float32)
    n = v.shape[0]
    chunks = -(-n // CHUNK)
    t = np.zeros(chunks * CHUNK, dtype=np.float64)
    t[:n] = v.astype(np.float64)
    t = (t * t).reshape(chunks, CHUNK)
    half = CHUNK // 2
    while half:
        t = t[:, :half] + t[:, half:2 * half]
        half //= 2
    acc = np.float64(0.0)
    for c in range(chunks):
        acc = acc + t[c, 0]
    return float(acc)


def rnd(word, n):
    return ((int(word) >> 8) * int(n)) >> 24


def draw(seed, u, d):
    seed, ctr = int(seed) & U64, (((int(u) & U64) << 8) | d) & U64
    return [int(x) for x in philox4x32_10(ctr & 0xFFFFFFFF, ctr >> 32, 0, 0, seed & 0xFFFFFFFF, seed >> 32)]


def threshold(prob):
    return int(math.floor(float(np.float32(prob)) * 16777216.0))


class Bank(object):
    """rirs, noises: lists of 1-D float32 arrays; the quantities the contract fixes once per bank."""

    def __init__(self, rirs, noises, sample_frequency, snrs):
        self.rirs = [np.asarray(h, dtype=np.float32) for h in rirs]
        self.noises = [np.asarray(q, dtype=np.float32) for q in noises]
        self.snrs = [float(s) for s in snrs] if self.noises else []
        fs = float(sample_frequency)
        before, after = int(math.floor(0.001 * fs)), int(math.floor(0.05 * fs))
        self.meta = []
        for h in self.rirs:
            p = int(np.argmax(h))                                      # numpy: the first of several largest
            self.meta.append((h.shape[0], p, max(0, p - before), min(h.shape[0], p + after)))
        self.noise_power = [power_sum(q) / float(q.shape[0]) for q in self.noises]
        self.snr_gain = [math.pow(10.0, -s / 10.0) for s in self.snrs]


def plan(bank, seed, u, rir_prob=1.0, noise_prob=1.0):
    out = {"rir": None, "noise": None, "snr": None, "offset": None}
    w = draw(seed, u, 0)
    if bank.rirs and rnd(w[0], 1 << 24) < threshold(rir_prob):
        out["rir"] = rnd(w[1], len(bank.rirs))
    w = draw(seed, u, 1)
    if bank.noises and rnd(w[0], 1 << 24) < threshold(noise_prob):
        m = rnd(w[1], len(bank.noises))
        out.update(noise=m, snr=rnd(w[2], len(bank.snrs)), offset=rnd(w[3], bank.noises[m].shape[0]))
    return out


def convolve(x, h):
    """float32 of the ascending float64 sum over the taps that meet a sample, over the full length n + K - 1."""
    x64, h64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(h, dtype=np.float32).astype(np.float64)
    n, K = x64.shape[0], h64.shape[0]
    acc = np.zeros(n + K - 1, dtype=np.float64)
    for k in range(K):                                                 # output i takes its terms in the order k = 0, 1, ...
        acc[k:k + n] = acc[k:k + n] + h64[k] * x64                     # the product of two float32 values is exact in float64
    return acc.astype(np.float32)


def stages(x, bank, seed, u, rir_prob=1.0, noise_prob=1.0, normalize=True):
    """Every intermediate of the contract for one utterance: a dict with plan, p_in, y, p_sig, g, added (the float64 term g q, or None), z,
    s (or None) and out."""
    x = np.asarray(x)
    x = x.astype(np.float32)                                           # int16 -> float32 is exact
    n = x.shape[0]
    pl = plan(bank, seed, u, rir_prob, noise_prob)
    r = {"plan": pl, "y": x.copy(), "g": None, "added": None, "s": None}
    if n == 0:
        r.update(out=x.copy(), z=x.copy(), p_in=None, p_sig=None)
        return r
    p_in = power_sum(x) / float(n)
    p_sig = p_in
    if pl["rir"] is not None:
        h = bank.rirs[pl["rir"]]
        _, _, lo, hi = bank.meta[pl["rir"]]
        r["y"] = convolve(x, h)[:n]
        e = convolve(x, h[lo:hi])
        p_sig = power_sum(e) / float(e.shape[0])
    z = r["y"]
    if pl["noise"] is not None and bank.noise_power[pl["noise"]] > 0.0:
        q = bank.noises[pl["noise"]]
        g = np.sqrt((np.float64(bank.snr_gain[pl["snr"]]) * np.float64(p_sig)) / np.float64(bank.noise_power[pl["noise"]]))
        idx = (pl["offset"] + np.arange(n, dtype=np.int64)) % q.shape[0]
        added = g * q[idx].astype(np.float64)
        z = (r["y"].astype(np.float64) + added).astype(np.float32)
        r.update(g=float(g), added=added)
    out = z
    if normalize:
        p_out = power_sum(z) / float(n)
        if p_out > 0.0:
            s = np.sqrt(np.float64(p_in) / np.float64(p_out))
            out = (s * z.astype(np.float64)).astype(np.float32)
            r["s"] = float(s)
    r.update(p_in=p_in, p_sig=p_sig, z=z, out=out)
    return r


def reverberate(x, bank, seed, u, rir_prob=1.0, noise_prob=1.0, normalize=True):
    return stages(x, bank, seed, u, rir_prob, noise_prob, normalize)["out"]
