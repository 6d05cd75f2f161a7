"""numpy restatement of the pitch features (include/ctcn.h, ctcn_pitch and ctcn_pitch_process: Kaldi's compute-kaldi-pitch-feats and
process-kaldi-pitch-feats, steps 1 to 9): the definition the kernels and their host twins are held to.  Steps 1 to 7 are float64 sums in a
fixed order and reproduce the library bit for bit; step 8 exists in a float64 and a float32 form (their difference is the tolerance's
yardstick).  Nothing here calls the library."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as RR  # noqa: E402

OPTS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, preemphasis_coefficient=0.0, min_f0=50.0, max_f0=400.0,
            soft_min_f0=10.0, penalty_factor=0.1, lowpass_cutoff=1000.0, resample_frequency=4000.0, delta_pitch=0.005, nccf_ballast=7000.0,
            lowpass_filter_width=1, upsample_filter_width=5, snip_edges=True)
PROCESS_OPTS = dict(pitch_scale=2.0, pov_scale=2.0, pov_offset=0.0, delta_pitch_scale=10.0, delta_pitch_noise_stddev=0.005,
                    normalization_left_context=75, normalization_right_context=75, delta_window=2, delay=0, add_pov_feature=True,
                    add_normalized_log_pitch=True, add_delta_pitch=True, add_raw_log_pitch=False)
VAR_LANES = 256
f32, f64 = np.float32, np.float64


def options(**kw):
    assert not set(kw) - set(OPTS), set(kw) - set(OPTS)
    o = dict(OPTS, **kw)
    return {k: (float(f32(v)) if isinstance(OPTS[k], float) else int(v)) for k, v in o.items()}      # floats as the C struct holds them


class Plan(object):
    """Steps 2 and 5 and the tables of step 6."""

    def __init__(self, **kw):
        o = self.o = options(**kw)
        self.fs, self.rf = int(o["sample_frequency"]), int(o["resample_frequency"])
        rf = float(self.rf)
        self.W = int(rf * o["frame_length"] / 1000.0)
        self.shift = int(rf * o["frame_shift"] / 1000.0)
        ufw = o["upsample_filter_width"]
        half = ufw / (2.0 * rf)
        self.first = int(math.ceil(rf * (1.0 / o["max_f0"] - half)))
        self.last = int(math.floor(rf * (1.0 / o["min_f0"] + half)))
        self.nm = self.last - self.first + 1
        lags, lag, max_lag = [], f32(1.0 / o["max_f0"]), f32(1.0 / o["min_f0"])
        while lag <= max_lag:
            lags.append(lag)
            lag = f32(f64(lag) * (1.0 + o["delta_pitch"]))
        self.lags = np.asarray(lags, dtype=f32)
        self.S = S = len(lags)
        self.pitch = (f32(1.0) / self.lags).astype(f32)
        cutoff = rf / 2.0
        fw = ufw / (2.0 * cutoff)
        self.tap_first, self.tap_count, rows = np.zeros(S, np.int64), np.zeros(S, np.int64), []
        for i in range(S):
            t = float(self.lags[i]) - self.first / rf
            a, b = max(int(math.ceil(rf * (t - fw))), 0), min(int(math.floor(rf * (t + fw))), self.nm - 1)
            w = []
            for j in range(a, b + 1):
                d = t - j / rf
                win = 0.5 * (1 + math.cos(2 * math.pi * cutoff / ufw * d)) if abs(d) < fw else 0.0
                filt = math.sin(2 * math.pi * cutoff * d) / (math.pi * d) if d != 0 else 2 * cutoff
                w.append(filt * win / rf)
            self.tap_first[i], self.tap_count[i] = a, b - a + 1
            rows.append(w)
        self.taps = int(self.tap_count.max())
        self.weights = np.zeros((S, self.taps), dtype=f32)
        for i, w in enumerate(rows):
            self.weights[i, :len(w)] = np.asarray(w, dtype=f64).astype(f32)
        self.soft_lag = f64(o["soft_min_f0"]) * self.lags.astype(f64)
        lg = math.log(1.0 + o["delta_pitch"])
        self.c = (lg * lg) * o["penalty_factor"]
        d = np.arange(S, dtype=f64)
        self.penalty = (d * d) * self.c
        self.nccf_ballast = o["nccf_ballast"]

    def downsampled(self, n):
        return RR.num_samples(n, self.fs, self.rf)

    def num_frames(self, n):
        m = self.downsampled(n)
        return 0 if m < self.W else (m - self.W) // self.shift + 1


def fbank_frames(n, length=400, shift=160):
    return 0 if n < length else (n - length) // shift + 1


def downsample(plan, wave):
    """Step 1: the resampler's restatement with the pitch extractor's filter."""
    o = plan.o
    first, ntaps, table = RR.weight_table(plan.fs, plan.rf, o["lowpass_filter_width"], o["lowpass_cutoff"])
    return RR.resample(np.asarray(wave), plan.fs, plan.rf, first, ntaps, table)


def ballast(plan, x):
    """(var W)^2 nccf_ballast: 256 partial sums, partial i over samples i, i + 256, ... in order, added in ascending order."""
    m = x.shape[0]
    xp = np.zeros(-(-m // VAR_LANES) * VAR_LANES, dtype=f64)             # adding +0.0 changes no bit of a sum that started at +0.0
    xp[:m] = x.astype(f64)
    rows = xp.reshape(-1, VAR_LANES)
    s, q = np.zeros(VAR_LANES, f64), np.zeros(VAR_LANES, f64)
    for r in rows:
        s = s + r
        q = q + r * r
    ts = tq = f64(0.0)
    for i in range(VAR_LANES):
        ts = ts + s[i]
        tq = tq + q[i]
    mean = ts / f64(m)
    var = tq / f64(m) - mean * mean
    vw = var * f64(plan.W)
    return (vw * vw) * f64(plan.nccf_ballast)


def nccf(plan, x):
    """Steps 3 to 5 on the downsampled signal x (M) float32: (nccf_pitch, nccf_pov), both (T, S) float32."""
    m, W, sh, S = x.shape[0], plan.W, plan.shift, plan.S
    T = 0 if m < W else (m - W) // sh + 1
    if T == 0:
        return np.zeros((0, S), f32), np.zeros((0, S), f32)
    win = W + plan.last
    xp = np.zeros((T - 1) * sh + win, dtype=f64)
    k = min(m, xp.shape[0])
    xp[:k] = x[:k].astype(f64)
    fr = xp[np.arange(T)[:, None] * sh + np.arange(win)[None, :]]        # (T, win)
    s = np.zeros(T, f64)
    for i in range(W):
        s = s + fr[:, i]
    mean = s / f64(W)
    v = fr - mean[:, None]
    e1 = np.zeros(T, f64)
    for i in range(W):
        e1 = e1 + v[:, i] * v[:, i]
    lag = np.arange(plan.first, plan.last + 1)
    e2, inner = np.zeros((T, plan.nm), f64), np.zeros((T, plan.nm), f64)
    for i in range(W):
        b = v[:, lag + i]
        e2 = e2 + b * b
        inner = inner + v[:, i:i + 1] * b
    prod = e1[:, None] * e2
    bal = ballast(plan, x)
    dp, dv = np.sqrt(prod + bal), np.sqrt(prod)
    with np.errstate(divide="ignore", invalid="ignore"):
        n_pitch = np.where(dp != 0.0, inner / dp, 0.0)
        n_pov = np.where(dv != 0.0, inner / dv, 0.0)
    out = []
    w64 = plan.weights.astype(f64)
    for rows in (n_pitch, n_pov):
        acc = np.zeros((T, S), f64)
        for j in range(plan.taps):
            ok = j < plan.tap_count
            col = np.minimum(plan.tap_first + j, plan.nm - 1)
            p = w64[:, j][None, :] * rows[:, col]
            acc = np.where(ok[None, :], acc + p, acc)
        out.append(acc.astype(f32))
    return out[0], out[1]


def viterbi(plan, n_pitch):
    """Step 6: the lag index per frame (T) for nccf_pitch (T, S) float32."""
    T, S = n_pitch.shape
    idx = np.abs(np.arange(S)[:, None] - np.arange(S)[None, :])
    pen = plan.penalty[idx]                                             # (i, j)
    prev = np.zeros(S, f64)
    bp = np.zeros((T, S), np.int64)
    for t in range(T):
        n = n_pitch[t].astype(f64)
        local = (1.0 - n) + plan.soft_lag * n
        cand = prev[None, :] + pen
        arg = cand.argmin(axis=1)                                       # the first (lowest j) of equal minima
        fwd = local + cand[np.arange(S), arg]
        bp[t] = arg
        prev = fwd - fwd.min()
    path = np.zeros(T, np.int64)
    if T:
        state = int(prev.argmin())
        for t in range(T - 1, -1, -1):
            path[t] = state
            if t > 0:
                state = int(bp[t, state])
    return path


def extract_downsampled(plan, x):
    """Steps 3 to 7 on the downsampled signal: (raw (T, 2) float32, lag indices (T))."""
    n_pitch, n_pov = nccf(plan, np.asarray(x, dtype=f32))
    path = viterbi(plan, n_pitch)
    T = path.shape[0]
    raw = np.zeros((T, 2), f32)
    raw[:, 0] = n_pov[np.arange(T), path]
    raw[:, 1] = plan.pitch[path]
    return raw, path


def extract(plan, wave):
    """Steps 1 to 7 on a waveform at sample_frequency (int16 or float32)."""
    return extract_downsampled(plan, downsample(plan, wave))


def delta_scales(window):
    """Kaldi's order-1 delta filter in float32 (ctcn_delta_scales)."""
    j = np.arange(-window, window + 1)
    norm = f32(0.0)
    for v in j:
        norm = f32(norm + f32(v * v))
    inv = f32(1.0 / f64(norm))
    return (j.astype(f32) * inv).astype(f32)


def gauss(seed, utt, frames):
    """The unit Gaussians of frames [0, frames) of utterance `utt`: Philox keyed as the filterbank's dither, sample 0 (the cosine)."""
    from oracle import philox
    ctr = (np.uint64(utt) << np.uint64(38)) | (np.arange(frames, dtype=np.uint64) << np.uint64(10))
    zero = np.zeros(frames, np.uint64)
    w = philox.philox4x32_10(ctr & philox.MASK, ctr >> np.uint64(32), zero, zero, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u1 = ((w[0] >> np.uint32(8)).astype(f32) + f32(1.0)) * f32(2.0 ** -24)
    th = f32(6.28318530717958647692) * ((w[1] >> np.uint32(8)).astype(f32) * f32(2.0 ** -24))
    return (np.sqrt(f32(-2.0) * np.log(u1)) * np.cos(th)).astype(f32)


def process(raw, dtype=f64, seed=0, utt=0, **kw):
    """Step 8 in `dtype` arithmetic: (T, C) of that dtype."""
    assert not set(kw) - set(PROCESS_OPTS), set(kw) - set(PROCESS_OPTS)
    o = dict(PROCESS_OPTS, **kw)
    assert o["delay"] == 0
    d = dtype
    raw = np.asarray(raw, dtype=f32)
    T = raw.shape[0]
    n, p = raw[:, 0].astype(d), raw[:, 1].astype(d)
    cols = []
    lp = np.log(p)
    if o["add_pov_feature"]:
        cols.append(d(f32(o["pov_scale"])) * (np.power(d(1.0001) - np.clip(n, d(-1), d(1)), d(0.15)) - d(1)) + d(f32(o["pov_offset"])))
    if o["add_normalized_log_pitch"]:
        a = np.minimum(np.abs(n), d(1))
        r = d(-5.2) + d(5.4) * np.exp(d(7.5) * (a - d(1))) + d(4.8) * a - d(2) * np.exp(d(-10) * a) + d(4.2) * np.exp(d(20) * (a - d(1)))
        pov = d(1) / (d(1) + np.exp(-r))
        out = np.zeros(T, d)
        left, right = o["normalization_left_context"], o["normalization_right_context"]
        for t in range(T):
            u0, u1 = max(t - left, 0), min(t + right, T - 1)
            s0 = s1 = d(0)
            for u in range(u0, u1 + 1):
                s0 = s0 + pov[u]
                s1 = s1 + pov[u] * lp[u]
            out[t] = d(f32(o["pitch_scale"])) * (lp[t] - s1 / s0)
        cols.append(out)
    if o["add_delta_pitch"]:
        w = o["delta_window"]
        sc = delta_scales(w).astype(d)
        dl = np.zeros(T, d)
        for k in range(-w, w + 1) if T else ():
            dl = dl + sc[k + w] * lp[np.clip(np.arange(T) + k, 0, T - 1)]
        std = f32(o["delta_pitch_noise_stddev"])
        if std > 0 and T:
            dl = dl + d(std) * gauss(seed, utt, T).astype(d)
        cols.append(d(f32(o["delta_pitch_scale"])) * dl)
    if o["add_raw_log_pitch"]:
        cols.append(lp)
    return np.stack(cols, axis=1).astype(d) if T else np.zeros((0, len(cols)), d)


def paste(a, b, tolerance=2):
    """Step 9: paste-feats --length-tolerance on two (T, F) matrices."""
    if abs(a.shape[0] - b.shape[0]) > tolerance:
        raise ValueError("lengths %d and %d differ by more than %d" % (a.shape[0], b.shape[0], tolerance))
    T = min(a.shape[0], b.shape[0])
    return np.concatenate([a[:T], b[:T]], axis=1)


def harmonic_tone(f0, seconds=1.0, rate=16000, harmonics=5, amplitude=1.0):
    t = np.arange(int(seconds * rate)) / rate
    return (amplitude * sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, harmonics + 1))).astype(f32)
