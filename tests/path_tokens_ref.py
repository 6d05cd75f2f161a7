"""numpy restatement of ctcn_path_tokens (the definition in include/ctcn.h), one frame at a time: what tests/test_path_tokens.py compares the
kernel with.  Integers and the minimum are exact; the sums are float64 in frame order, rounded once to float32."""
import numpy as np


def path_tokens(path_bt, lens, lp, blank=0):
    """path_bt (B, T) integers, lens (B), lp (T, B, V) float32 -> dict of ids, starts, ends (B, T) int32 (-1 past lengths), lengths (B) int32,
    mean_lp, min_lp, mean_margin (B, T) float32 (0 past lengths), path_score (B) float32."""
    path_bt, lp = np.asarray(path_bt), np.asarray(lp, dtype=np.float32)
    T, B, V = lp.shape
    assert path_bt.shape == (B, T) and 0 <= blank < V
    ids, starts, ends = (np.full((B, T), -1, dtype=np.int32) for _ in range(3))
    mean, mn, margin = (np.zeros((B, T), dtype=np.float32) for _ in range(3))
    lengths, score = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        valid = [0 <= int(path_bt[b, t]) < V for t in range(n)]
        k = [int(path_bt[b, t]) if valid[t] else blank for t in range(n)]           # an id outside [0, V) counts as blank ...
        total, j, t = 0.0, 0, 0
        for u in range(n):
            if valid[u]:                                                            # ... and never indexes lp
                total += float(lp[u, b, k[u]])
        while t < n:
            if k[t] == blank or (t > 0 and k[t] == k[t - 1]):
                t += 1
                continue
            e = t + 1
            while e < n and k[e] == k[t]:
                e += 1
            own = lp[t:e, b, k[t]].astype(np.float64)
            others = np.delete(lp[t:e, b, :], k[t], axis=1)
            best = others.max(axis=1).astype(np.float64) if V > 1 else np.full(e - t, -np.inf)
            with np.errstate(invalid="ignore"):
                ids[b, j], starts[b, j], ends[b, j] = k[t], t, e
                mean[b, j] = np.float32(sum(own.tolist()) / (e - t))
                mn[b, j] = lp[t:e, b, k[t]].min()
                margin[b, j] = np.float32(sum((own - best).tolist()) / (e - t))
            j += 1
            t = e
        lengths[b], score[b] = j, np.float32(total)
    return {"ids": ids, "lengths": lengths, "starts": starts, "ends": ends, "mean_lp": mean, "min_lp": mn, "mean_margin": margin,
            "path_score": score}
