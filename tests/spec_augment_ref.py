"""SpecAugment as include/ctcn.h specifies it, restated in numpy on top of oracle.philox.philox4x32_10  --  TEST INFRASTRUCTURE ONLY.

Written from the text of the contract, not from specaug.hip:

    T = the utterance's frames, u = its 64-bit index, draw(d) = philox4(seed, (u << 8) | d): counter (lo32, hi32, 0, 0), key = seed
    rnd(word, n) = ((word >> 8) * n) >> 24                                                  (integers only)
    warp  (d = 0, W > 0 and T > 2 W):  c = W + rnd(r0, T - 2 W), w = c + rnd(r1, 2 W - 1) - (W - 1)
          row t < w reads position t c / w, row t >= w reads c + (t - w)(T - c) / (T - w): integer quotient i0, remainder rem,
          i1 = min(i0 + 1, T - 1); rem = 0: x[i0]; else a = rem / den in float64 and float32((1 - a) x[i0] + a x[i1]), each operation
          rounded on its own (numpy never fuses)
    freq  (d = 1 .. nf):  len = rnd(r0, min(freq_width, F) + 1), f0 = rnd(r1, F - len + 1)
    time  (d = 9 + k):    cap = min(time_width, T, floor(float64(float32(time_ratio)) T)), len = rnd(r0, cap + 1), t0 = rnd(r1, T - len + 1)
    out[t][f] = fill inside any mask of the WARPED output, else the warped value; rows >= T of a padded batch are zeros."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.philox import philox4x32_10  # noqa: E402

U64 = (1 << 64) - 1
OPTION_NAMES = ("warp_window", "num_freq_masks", "freq_width", "num_time_masks", "time_width", "time_ratio", "fill")
DEFAULTS = dict(warp_window=5, num_freq_masks=2, freq_width=15, num_time_masks=2, time_width=40, time_ratio=0.2)


def options(**kw):
    o = dict(warp_window=0, num_freq_masks=0, freq_width=0, num_time_masks=0, time_width=0, time_ratio=1.0, fill=0.0)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def draw(seed, u, d):
    seed, ctr = int(seed) & U64, (((int(u) & U64) << 8) | d) & U64
    w = philox4x32_10(ctr & 0xFFFFFFFF, ctr >> 32, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    return [int(x) for x in w]


def rnd(word, n):
    return ((word >> 8) * n) >> 24


def plan(T, F, seed, u, **kw):
    """{"warp": (c, w) | None, "freq": [(f0, len)], "time": [(t0, len)]}"""
    o = options(**kw)
    W = o["warp_window"]
    warp = None
    if W > 0 and T > 2 * W:
        r = draw(seed, u, 0)
        c = W + rnd(r[0], T - 2 * W)
        warp = (c, c + rnd(r[1], 2 * W - 1) - (W - 1))
    freq = []
    for k in range(o["num_freq_masks"]):
        r = draw(seed, u, 1 + k)
        n = rnd(r[0], min(o["freq_width"], F) + 1)
        freq.append((rnd(r[1], F - n + 1), n))
    time = []
    for k in range(o["num_time_masks"]):
        r = draw(seed, u, 9 + k)
        cap = min(o["time_width"], T, int(math.floor(float(np.float64(np.float32(o["time_ratio"])) * np.float64(T)))))
        n = rnd(r[0], cap + 1)
        time.append((rnd(r[1], T - n + 1), n))
    return {"warp": warp, "freq": freq, "time": time}


def warp_rows(x, c, w):
    """The warped utterance: x (T, F) float32 -> (T, F) float32."""
    T = x.shape[0]
    out = np.empty_like(x)
    for t in range(T):
        if t < w:
            num, den, base = t * c, w, 0
        else:
            num, den, base = (t - w) * (T - c), T - w, c
        i0, rem = base + num // den, num % den
        i1 = min(i0 + 1, T - 1)
        if rem == 0:
            out[t] = x[i0]
        else:
            a = np.float64(rem) / np.float64(den)
            out[t] = ((np.float64(1.0) - a) * x[i0].astype(np.float64) + a * x[i1].astype(np.float64)).astype(np.float32)
    return out


def augment(x, seed, u, **kw):
    """One utterance x (T, F) float32 -> its augmented (T, F) float32."""
    x = np.asarray(x, dtype=np.float32)
    T, F = x.shape
    p = plan(T, F, seed, u, **kw)
    out = warp_rows(x, *p["warp"]) if p["warp"] else x.copy()
    fill = np.float32(options(**kw)["fill"])
    for f0, n in p["freq"]:
        out[:, f0:f0 + n] = fill
    for t0, n in p["time"]:
        out[t0:t0 + n] = fill
    return out


def augment_batch(utts, seed, utt_offset, Tmax=None, **kw):
    """A list of utterances -> the padded (B, Tmax, F) batch the kernel writes: zeros behind every utterance."""
    Tmax = max(u.shape[0] for u in utts) if Tmax is None else Tmax
    out = np.zeros((len(utts), Tmax, utts[0].shape[1]), dtype=np.float32)
    for b, x in enumerate(utts):
        out[b, :x.shape[0]] = augment(x, seed, utt_offset + b, **kw)
    return out
