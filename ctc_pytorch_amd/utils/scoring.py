"""Error breakdown scoring: what lies behind the single error rate the recipe reports.

`ErrorStats` accumulates the six totals of ops.edit_ops / ctcn_levenshtein_ops (sub, del, ins, cor, hypothesis length, reference length) and
the (V+1, V+1) confusion table (row V: insertions by hypothesis class, column V: deletions by reference class) in ONE flat int64 tensor, on
the device or on the host, and prints the standard `%PER x.xx [ e / n, i ins, d del, s sub ]` line with the top confusions by name.
`load_phone_map` reads the reference's three-column fold table (conf/phones.60-48-39.map, applied there at data-preparation time by
local/normalize_phone.py --to 60-48|60-39|48-39) into the class map those entry points take, so that a model trained on 48 or 60 classes is
scored on 39 -- the TIMIT convention.  `align_ids` is the host alignment (library host code, no GPU needed)."""
import numpy as np
import torch

N_TOTALS = 6
_COLS = {"60-48": (0, 1), "60-39": (0, 2), "48-39": (1, 2)}


def _names(index2word):
    """{id: name} of a vocabulary given as a dict or a sequence, and V = largest id + 1."""
    items = dict(index2word.items() if isinstance(index2word, dict) else enumerate(index2word))
    items = {int(k): w for k, w in items.items()}
    return items, (max(items) + 1 if items else 0)


def load_phone_map(path, cols, index2word):
    """The class map (int32, V entries) of the fold `cols` ("60-48", "60-39" or "48-39") of a three-column phone table: the phone named in
    the source column becomes the phone named in the target column, a line without the target column drops its phone (-1, as `q` is), names
    absent from the file (the blank, for one) map to themselves.  A target name outside the vocabulary raises ValueError."""
    if cols not in _COLS:
        raise ValueError("load_phone_map: cols must be one of %s, got %r" % (sorted(_COLS), cols))
    src, tgt = _COLS[cols]
    names, V = _names(index2word)
    ids = {}
    for k in sorted(names):
        ids.setdefault(names[k], k)
    table = {}
    with open(path, "r") as f:
        for line in f:
            parts = line.split()
            if len(parts) > src:
                table[parts[src]] = parts[tgt] if len(parts) > tgt else None
    out = np.arange(V, dtype=np.int32)
    for k, name in names.items():
        if name not in table:
            continue
        to = table[name]
        if to is None:
            out[k] = -1
        elif to not in ids:
            raise ValueError("load_phone_map: %r maps to %r, which the vocabulary does not hold" % (name, to))
        else:
            out[k] = ids[to]
    return out


def align_ids(hyp, ref, class_map=None, alignment=True):
    """Host alignment of two id sequences (ctcn_levenshtein_ops, the move rule of ops.edit_ops): ((sub, del, ins, cor), pairs) with pairs an
    (n, 2) int32 array of (reference id, hypothesis id), -1 = none (None with alignment=False).  class_map as in ops.edit_ops."""
    from ctc_pytorch_amd import _lib

    def mapped(seq):
        seq = np.asarray(seq, dtype=np.int64).reshape(-1)
        if class_map is not None and seq.size:
            cm = np.asarray(class_map, dtype=np.int64)
            inside = (seq >= 0) & (seq < cm.size)
            seq = np.where(inside, cm[np.where(inside, seq, 0)], seq)
            seq = seq[~(inside & (seq == -1))]
        return np.ascontiguousarray(seq, dtype=np.int32)

    h, r = mapped(hyp), mapped(ref)
    counts = np.zeros(4, dtype=np.int64)
    ali = np.empty((len(h) + len(r), 2), dtype=np.int32) if alignment else None
    n = _lib.lib().ctcn_levenshtein_ops(h.ctypes.data if len(h) else None, len(h), r.ctypes.data if len(r) else None, len(r),
                                        counts.ctypes.data, ali.ctypes.data if ali is not None and ali.size else None)
    if n < 0:
        raise RuntimeError("ctcn_levenshtein_ops failed (%d)" % n)
    return tuple(int(c) for c in counts), (ali[:n] if ali is not None else None)


class ErrorStats(object):
    """Running error breakdown over a test set.  One flat int64 tensor: the six totals, then the (V+1) x (V+1) confusion table row by row --
    data-parallel ranks sum it with a single all-reduce (`state` / `from_state` / `merge`).  With device= a ROCm device the accumulators live
    there: `confusion` is the view ops.edit_ops(confusion=) adds into and `add(counts)` is a device sum, so a scoring loop never waits for
    the device; `totals` / `report` make the one copy to the host."""

    def __init__(self, index2word, device=None):
        self.names, self.V = _names(index2word)
        self._state = torch.zeros(N_TOTALS + (self.V + 1) ** 2, dtype=torch.int64, device=device)

    @property
    def confusion(self):
        return self._state[N_TOTALS:].view(self.V + 1, self.V + 1)

    def add(self, counts=None, confusion=None):
        """counts: (B, 6) or (6,) as ops.edit_ops returns them, or (B, 4) / (4,) (sub, del, ins, cor) of the host alignment, whose lengths
        follow from the invariants; confusion: a (V+1, V+1) table to add (not the `confusion` view itself: that one is added into in place)."""
        if counts is not None:
            c = torch.as_tensor(counts).to(device=self._state.device, dtype=torch.int64).reshape(-1, np.shape(counts)[-1]).sum(0)
            if c.numel() == 4:
                c = torch.cat([c, (c[0] + c[2] + c[3]).reshape(1), (c[0] + c[1] + c[3]).reshape(1)])
            if c.numel() != N_TOTALS:
                raise ValueError("ErrorStats.add: counts must have 6 (or 4) columns")
            self._state[:N_TOTALS] += c
        if confusion is not None:
            t = torch.as_tensor(confusion).to(device=self._state.device, dtype=torch.int64)
            if tuple(t.shape) != (self.V + 1, self.V + 1):
                raise ValueError("ErrorStats.add: confusion must be (%d, %d)" % (self.V + 1, self.V + 1))
            self._state[N_TOTALS:] += t.reshape(-1)
        return self

    def add_pairs(self, counts4, pairs):
        """One host alignment (align_ids): its four counts and its (reference, hypothesis) pairs; pairs with a member outside [0, V) are
        counted but not entered, as on the device."""
        self.add(counts4)
        if pairs is not None and len(pairs):
            V = self.V
            r, h = np.asarray(pairs[:, 0], dtype=np.int64), np.asarray(pairs[:, 1], dtype=np.int64)
            ok = np.where(r == -1, (h >= 0) & (h < V), np.where(h == -1, (r >= 0) & (r < V), (r >= 0) & (r < V) & (h >= 0) & (h < V)))
            # (a pair says "none" with -1, so an id of -1 on the host cannot be told from it here; the decoders and the drivers produce none)
            flat = np.where(r == -1, V, r)[ok] * (V + 1) + np.where(h == -1, V, h)[ok]
            add = torch.from_numpy(np.bincount(flat, minlength=(V + 1) ** 2).astype(np.int64))
            self._state[N_TOTALS:] += add.to(self._state.device)
        return self

    def merge(self, other):
        if other.V != self.V:
            raise ValueError("ErrorStats.merge: %d classes here, %d there" % (self.V, other.V))
        self._state += other._state.to(self._state.device)
        return self

    def state(self):
        return self._state.clone()

    @classmethod
    def from_state(cls, index2word, state):
        out = cls(index2word, device=state.device if torch.is_tensor(state) else None)
        state = torch.as_tensor(state).to(torch.int64).reshape(-1)
        if state.numel() != out._state.numel():
            raise ValueError("ErrorStats.from_state: %d values for %d classes (%d expected)" % (state.numel(), out.V, out._state.numel()))
        out._state.copy_(state)
        return out

    def _host(self):
        s = self._state.cpu().numpy()                    # the one copy
        return s[:N_TOTALS], s[N_TOTALS:].reshape(self.V + 1, self.V + 1)

    def totals(self):
        t, _ = self._host()
        sub, dele, ins, cor, nh, nr = (int(v) for v in t)
        err = sub + dele + ins
        return dict(sub=sub, ins=ins, cor=cor, hyp_len=nh, ref_len=nr, errors=err, per=100.0 * err / max(nr, 1), **{"del": dele})

    @staticmethod
    def summary_line(sub, dele, ins, ref_len, tag="%PER"):
        err = sub + dele + ins
        return "%s %.2f [ %d / %d, %d ins, %d del, %d sub ]" % (tag, 100.0 * err / max(ref_len, 1), err, ref_len, ins, dele, sub)

    def report(self, top=10, tag="%PER"):
        t, tab = self._host()
        V = self.V
        name = lambda k: str(self.names.get(int(k), "<%d>" % int(k)))
        lines = [self.summary_line(int(t[0]), int(t[1]), int(t[2]), int(t[5]), tag)]

        def ranked(values, keys):
            order = sorted(range(len(values)), key=lambda n: (-int(values[n]), keys[n]))
            return [(keys[n], int(values[n])) for n in order[:top] if values[n] > 0]

        off = tab[:V, :V].copy()
        np.fill_diagonal(off, 0)
        rr, hh = np.nonzero(off)
        subs = ranked(off[rr, hh], list(zip(rr.tolist(), hh.tolist())))
        lines.append("confusions (reference -> hypothesis): " + (", ".join("%s -> %s %d" % (name(r), name(h), n) for (r, h), n in subs) or "none"))
        lines.append("deletions: " + (", ".join("%s %d" % (name(k), n) for k, n in ranked(tab[:V, V], list(range(V)))) or "none"))
        lines.append("insertions: " + (", ".join("%s %d" % (name(k), n) for k, n in ranked(tab[V, :V], list(range(V)))) or "none"))
        return "\n".join(lines)
