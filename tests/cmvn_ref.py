"""numpy restatement of the grouped and the sliding-window mean / variance normalisation, written from the contract in include/ctcn.h (not
from the kernels): the grouped sums in the stated order, mean and scale, the window rule, the running sums -- every float64 operation a
numpy operation of its own, so nothing is fused.  sliding_kaldi is the same normalisation in the arithmetic of Kaldi's SlidingWindowCmn
(float32 output, x + (-1 / w) S, variance as Q / w - S^2 / w^2 and pow(-0.5)); Kaldi's binaries do not run here, so the two are compared
within a derived bound, not bit for bit."""
import numpy as np

ROWS = 64           # rows of one partial sum of ctcn_cmvn_accumulate


def accumulate_groups(feats, frames, groups, stats):
    """stats (G, 2, F + 1) float64 with the rows t < frames[b] of feats (B, Tmax, F) float32 added to stats[groups[b]]: per 64-row block
    ascending float64 sums of x and x * x; per group the blocks of its utterances added in ascending (utterance, block) order, from 0, and
    that sum added to stats; the frame counts in ascending utterance order.  An id outside [0, G) contributes nothing."""
    B, Tmax, F = feats.shape
    G = stats.shape[0]
    out = stats.copy()
    for g in range(G):
        s, q, cnt = np.zeros(F, np.float64), np.zeros(F, np.float64), np.float64(0.0)
        for b in range(B):
            if int(groups[b]) != g:
                continue
            n = min(max(int(frames[b]), 0), Tmax)
            for t0 in range(0, Tmax, ROWS):
                ps, pq = np.zeros(F, np.float64), np.zeros(F, np.float64)
                for t in range(t0, min(t0 + ROWS, n)):
                    v = feats[b, t].astype(np.float64)
                    ps = ps + v
                    pq = pq + v * v
                s = s + ps
                q = q + pq
            cnt = cnt + np.float64(n)
        out[g, 0, :F] = out[g, 0, :F] + s
        out[g, 1, :F] = out[g, 1, :F] + q
        out[g, 0, F] = out[g, 0, F] + cnt
    return out


def mean_scale(stats, norm_vars=True):
    """(mean, scale) float32 of one (2, F + 1) matrix: m = sum / n, v = max(sumsq / n - m * m, 1e-20), scale = 1 / sqrt(v)."""
    n = stats[0, -1]
    m = stats[0, :-1] / n
    if not norm_vars:
        return m.astype(np.float32), np.ones(m.shape, np.float32)
    mm = m * m
    v = np.maximum(stats[1, :-1] / n - mm, 1e-20)
    return m.astype(np.float32), (1.0 / np.sqrt(v)).astype(np.float32)


def apply(feats, frames, stats, groups=None, norm_vars=True):
    """(x - mean) * scale in float32 per utterance with its group's statistics; zeros at and beyond frames[b]; an id outside [0, G) or a
    group without frames copies the utterance through."""
    B, Tmax, F = feats.shape
    G = stats.shape[0]
    out = np.zeros((B, Tmax, F), np.float32)
    for b in range(B):
        n = min(max(int(frames[b]), 0), Tmax)
        g = 0 if groups is None else int(groups[b])
        x = feats[b, :n]
        if 0 <= g < G and stats[g, 0, F] > 0:
            mean, scale = mean_scale(stats[g], norm_vars)
            d = (x - mean).astype(np.float32)
            out[b, :n] = (d * scale).astype(np.float32)
        else:
            out[b, :n] = x
    return out


def window(t, n, cmn_window=600, min_cmn_window=100, center=False):
    """[s, e) of frame t in an utterance of n frames: the four steps of the contract."""
    if center:
        s = t - cmn_window // 2
        e = s + cmn_window
    else:
        s = t - cmn_window
        e = t + 1
    if s < 0:
        e -= s
        s = 0
    if not center and e > t:
        e = max(t + 1, min_cmn_window)
    if e > n:
        s -= e - n
        e = n
        s = max(s, 0)
    return s, e


def sliding(x, cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False):
    """x (n, F) float32 -> (n, F) float32 by the running float64 sums of the contract, all columns at once."""
    n, F = x.shape
    out = np.zeros((n, F), np.float32)
    if n == 0:
        return out
    xd = x.astype(np.float64)
    s, e = window(0, n, cmn_window, min_cmn_window, center)
    S, Q = np.zeros(F, np.float64), np.zeros(F, np.float64)
    for u in range(s, e):
        S = S + xd[u]
        Q = Q + xd[u] * xd[u]
    for t in range(n):
        if t > 0:
            s1, e1 = window(t, n, cmn_window, min_cmn_window, center)
            assert 0 <= s1 - s <= 1 and 0 <= e1 - e <= 1
            if s1 > s:
                S = S - xd[s]
                Q = Q - xd[s] * xd[s]
            if e1 > e:
                S = S + xd[e]
                Q = Q + xd[e] * xd[e]
            s, e = s1, e1
        w = np.float64(e - s)
        m = S / w
        d = xd[t] - m
        if normalize_variance and e - s > 1:
            mm = m * m
            v = np.maximum(Q / w - mm, 1e-10)
            inv = 1.0 / np.sqrt(v)
            d = d * inv
        out[t] = d.astype(np.float32)
    return out


def sliding_kaldi(x, cmn_window=600, min_cmn_window=100, normalize_variance=False, center=False):
    """The same in Kaldi's arithmetic (SlidingWindowCmnInternal): float64 running sums, the output row a float32 copy of the input updated as
    x + float32(-1 / w) * S (one rounding to float32); the variance Q / w - S^2 / w^2 in double, floored at 1e-10, raised to -0.5 and
    multiplied onto the float32 row (a second rounding to float32)."""
    n, F = x.shape
    out = np.zeros((n, F), np.float32)
    if n == 0:
        return out
    xd = x.astype(np.float64)
    ps = pe = 0
    S, Q = np.zeros(F, np.float64), np.zeros(F, np.float64)
    for t in range(n):
        s, e = window(t, n, cmn_window, min_cmn_window, center)
        if t == 0:
            for u in range(s, e):
                S = S + xd[u]
                Q = Q + xd[u] * xd[u]
        else:
            if s > ps:
                S = S - xd[ps]
                Q = Q - xd[ps] * xd[ps]
            if e > pe:
                S = S + xd[pe]
                Q = Q + xd[pe] * xd[pe]
        ps, pe = s, e
        w = e - s
        alpha = np.float64(np.float32(-1.0 / w))                        # AddVec(float alpha, double vector): the product and the sum in double
        row = (xd[t] + alpha * S).astype(np.float32)
        if normalize_variance and w > 1:
            var = Q * (1.0 / w) + (S * S) * (-1.0 / (w * w))
            var = np.maximum(var, 1e-10) ** -0.5
            row = (row.astype(np.float64) * var).astype(np.float32)    # MulElements(double vector) on the float32 row
        out[t] = row
    return out
