"""The CTC prefix beam search with an LM of order 2 or 3, restated in plain Python -- the checker of tests/test_beam_trigram*.py.

The search is the reference's ctcBeamSearch.decode as oracle/beam_ref.c states it (double ln domain, the LOG_ZERO rules of log_add_prob, the
float32 skip and repeat compares, dict-order merging, the stable sort, status 1 / 2 for its IndexError / ValueError); the one term that
changes is the LM term of calcExtPr and of the final step.  With a 3-D table tri[c0][c1][k] (index V = '<s>' for c0 and c1, '</s>' for k) a
labelling y extended by k, or closed by '</s>', takes
    len(y) == 0: tri[V][V][k]        len(y) == 1: tri[V][y[0]][k]        len(y) >= 2: tri[y[-2]][y[-1]][k]
and with a 2-D table lm[c1][k] it is the bigram search, bit for bit the C oracle's (tests/test_beam_trigram_host.py holds it to that on
the golden decoder sets, and under a context-free 3-D table).

How the dict of labellings is kept: two entries of a frame can only share a labelling when one is the stay entry of a labelling of the
beam and the other the extension of its parent, which is in the beam too.  Those few go through a dict as in the reference; every other
extension is a fresh entry (log_add_prob(LOG_ZERO, pr) = pr) that is only written out if the cut keeps it.  Positions are those of the
reference's dict: first touch.

Besides the result every utterance reports its GAP: the smallest relative distance between the last kept and the first dropped entry of
every cut `sort()[0:W]`, and between neighbours of the final sort.  A kernel whose scores differ from these in the last bits takes the same
decisions wherever that gap is far above those bits; a test compares utterances whose gap says so.
"""
import math

import numpy as np

LOG_ZERO = -99999999.0


def log_add_prob(log_x, log_y):
    if log_x <= LOG_ZERO:
        return log_y
    if log_y <= LOG_ZERO:
        return log_x
    if (log_y - log_x) > 0.0:
        log_x, log_y = log_y, log_x
    return log_x + math.log(1 + math.exp(log_y - log_x))


def _rel_gap(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0.0 else 0.0


class _Rows(object):
    """The LM row of a labelling: lm[c1] (order 2) or tri[c0][c1] (order 3) as a list of V + 1 floats."""

    def __init__(self, table, V):
        t = np.asarray(table, dtype=np.float64)
        if t.ndim == 2:
            t = t.reshape(V + 1, V + 1)
        assert t.shape == (V + 1,) * t.ndim and t.ndim in (2, 3), t.shape
        self.order, self.V, self.rows = t.ndim, V, t       # (rows as arrays: a beam entry's V extension scores are formed at once)

    def __call__(self, y):
        V = self.V
        if self.order == 2:
            return self.rows[y[-1] if y else V]
        if len(y) >= 2:
            return self.rows[y[-2]][y[-1]]
        return self.rows[V][y[0] if y else V]


def _cut(vals, W):
    """Positions of the first W entries of the stable descending sort, and the relative gap at the cut (inf: nothing is dropped)."""
    if len(vals) > 256:        # (numpy's stable sort of the negated values: the same order, faster on a long list)
        order = np.argsort(-np.asarray(vals, dtype=np.float64), kind="stable")[:W + 1].tolist()
    else:
        order = sorted(range(len(vals)), key=vals.__getitem__, reverse=True)
    gap = _rel_gap(vals[order[W - 1]], vals[order[W]]) if len(order) > W else math.inf
    return order[:W], gap


def _decode_one(mat, n, rows, alpha, W, blank, nbest):
    """mat (T, V) float32.  Returns (status, [(labelling, score)] best first, gap)."""
    V = mat.shape[1]
    one, tenth, nine = np.float32(1.0), np.float32(0.1), np.float32(0.9)
    ks = [k for k in range(V) if k != blank]
    # an entry of the beam: [labelling, prNonBlank, prBlank, prTotal]; `vals` / `refs` = prTotal and entry (or (parent entry, class, pr) of a
    # fresh extension) of every labelling of the frame, in first-touch order
    vals, refs = [0.0], [[(), LOG_ZERO, 0.0, 0.0]]
    gap = math.inf

    def beam():
        nonlocal gap
        keep, g = _cut(vals, W)
        gap = min(gap, g)
        out = []
        for i in keep:
            r = refs[i]
            if type(r) is tuple:
                r = [r[0][0] + (r[1],), r[2], LOG_ZERO, r[2]]
            out.append(r)
        return out

    for t in range(n):
        row = mat[t]
        if (one - row[blank]) < tenth:
            continue
        bhat = beam()
        if not all(p > 0.0 for p in row.tolist()):
            return 2, [], gap
        lg = [math.log(p) for p in row.astype(np.float64).tolist()]
        lgk = np.array(lg, dtype=np.float64)[ks]
        rep_ok = t > 0 and bool(mat[t - 1][blank] < nine)
        lgb = lg[blank]
        inbeam = {e[0] for e in bhat}
        kids = {}                                  # labelling of the beam -> classes whose extension is a labelling of the beam too
        for y in inbeam:
            if y and y[:-1] in inbeam:
                kids.setdefault(y[:-1], set()).add(y[-1])
        curr, slot = {}, {}
        vals, refs = [], []

        def touch(y):
            e = curr.get(y)
            if e is None:
                e = curr[y] = [y, LOG_ZERO, LOG_ZERO, LOG_ZERO]
                slot[y] = len(vals)
                vals.append(LOG_ZERO)
                refs.append(e)
            return e

        for e in bhat:
            y, prNB, prB, prT = e
            s_nb = prNB + lg[y[-1]] if y else LOG_ZERO
            s_b = prT + lgb
            c = touch(y)
            c[1] = log_add_prob(c[1], s_nb)
            c[2] = log_add_prob(c[2], s_b)
            c[3] = log_add_prob(c[3], log_add_prob(s_b, s_nb))
            lm = rows(y)
            prs = ((lgk + lm[ks] * alpha) + prT).tolist()           # lg[k] + lm[k] * alpha + prT per class: IEEE double, one rounding per operation
            if y and rep_ok:
                k = y[-1]
                prs[k if k < blank else k - 1] = lg[k] + float(lm[k]) * alpha + prB
            sp = kids.get(y)
            if not sp:
                vals.extend(prs)
                refs.extend([(e, k, pr) for k, pr in zip(ks, prs)])
                continue
            for k, pr in zip(ks, prs):
                if k in sp:
                    c = touch(y + (k,))
                    c[1] = log_add_prob(c[1], pr)
                    c[3] = log_add_prob(c[3], pr)
                else:
                    vals.append(pr)
                    refs.append((e, k, pr))
        for y, i in slot.items():
            vals[i] = curr[y][3]

    bhat = beam()
    if any(not e[0] for e in bhat):
        return 1, [], gap
    V_ = V
    fin = []
    for y, _, _, prT in bhat:
        pr = prT + float(rows(y)[V_]) * alpha
        fin.append(pr * (1.0 / len(y)))
    order = sorted(range(len(fin)), key=fin.__getitem__, reverse=True)
    for a, b in zip(order[:-1], order[1:]):
        gap = min(gap, _rel_gap(fin[a], fin[b]))
    return 0, [(list(bhat[i][0]), fin[i]) for i in order[:nbest]], gap


def decode(probs_tbv, lens, table, alpha, W, blank=0, nbest=0):
    """probs (T, B, V) float32 probabilities, table (V+1, V+1) or (V+1, V+1, V+1).  Returns what ops.beam_decode returns (nbest = 0: ids per
    utterance, scores (B,), status list) or what ops.beam_decode_nbest returns (nbest >= 1: lists of up to nbest labellings, scores
    (B, nbest)), and the gaps (B,)."""
    probs = np.asarray(probs_tbv, dtype=np.float32)
    T, B, V = probs.shape
    rows = _Rows(table, V)
    N = max(nbest, 1)
    ids, status, gaps = [], [], np.full(B, np.inf)
    score = np.zeros((B, N), dtype=np.float64)
    for b in range(B):
        st, best, gaps[b] = _decode_one(np.ascontiguousarray(probs[:, b]), min(max(int(lens[b]), 0), T), rows, float(alpha), int(W), int(blank), N)
        status.append(st)
        for k, (_, s) in enumerate(best):
            score[b, k] = s
        ids.append([y for y, _ in best] if nbest else (best[0][0] if best else []))
    return ids, (score if nbest else score[:, 0]), status, gaps


def context_free(lm2):
    """tri[c0] = the bigram table for every c0: the order-3 search over it is the order-2 search."""
    lm2 = np.asarray(lm2, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(lm2, (lm2.shape[0],) + lm2.shape))


def random_table(V, seed, blank=0, explicit=1.0 / 3.0):
    """A context-dependent table built the ARPA way: a random bigram table, random back-off weights per (c0, c1) and `explicit` of the
    entries drawn on their own; NaN where the search never reads (the blank's planes, rows and columns; c1 = <s> behind a class)."""
    rs = np.random.RandomState(seed)
    bi = -3.0 * rs.random_sample((V + 1, V + 1))
    bo = -1.0 * rs.random_sample((V + 1, V + 1, 1))
    tri = bo + bi[None, :, :]
    own = rs.random_sample(tri.shape) < explicit
    tri[own] = (-3.0 * rs.random_sample(tri.shape))[own]
    tri[V, V] = bi[V]
    return with_nans(tri, blank)


def with_nans(tri, blank):
    tri = np.array(tri, dtype=np.float64)
    V = tri.shape[0] - 1
    tri[blank], tri[:, blank], tri[:, :, blank] = np.nan, np.nan, np.nan
    tri[:V, V] = np.nan
    return tri


def blank_order(V, b):
    """old[j] = the class that sits at j once the blank has moved from class 0 to class b (the other classes keep their order)."""
    return np.array([c for c in range(1, b + 1)] + [0] + [c for c in range(b + 1, V)], dtype=np.int64)


def move_blank3(probs, tri, b):
    """synth.move_blank for a 3-D table: the blank from class 0 to class b, the other classes in order; returns (probs', tri', old)."""
    V = probs.shape[-1]
    old = blank_order(V, b)
    ext = np.concatenate([old, [V]])
    return np.ascontiguousarray(probs[..., old]), with_nans(np.asarray(tri)[np.ix_(ext, ext, ext)], b), old


# ---- the batches that tests/test_beam_trigram.py decodes on the GPU and tests/test_beam_trigram_host.py holds to the gap rule ----------
GAP = 1e-9            # relative; the suite's score gate is 4 spacings, ~1e-15
ALPHA = 0.5
_W62 = (1, 4, 20, 52, 60, 61, 130, 300)


def _specs():
    s = {}
    for regime in ("peaky", "flat"):
        for W in _W62:
            s["ctx62_%s_W%d" % (regime, W)] = dict(kind="random", V=62, T=48, B=8, regime=regime, W=W)
        for W in (4, 20, 61):
            s["ctx6_%s_W%d" % (regime, W)] = dict(kind="random", V=6, T=48, B=8, regime=regime, W=W)
        for W in (20, 130):
            s["nbest62_%s_W%d" % (regime, W)] = dict(kind="random", V=62, T=48, B=8, regime=regime, W=W, nbest=3)
    s["ctx62_flat_W1024"] = dict(kind="random", V=62, T=24, B=2, regime="flat", W=1024)
    # (V = 2: one class, labellings 1, 1 1, ...; from W = 4 on the first cuts fall among entries of LOG_ZERO + something, extensions of a
    # labelling that has no blank path yet under the repeat rule, whose relative distance is ~1e-9: no shape for this comparison)
    for W in (2, 3):
        s["ctx2_flat_W%d" % W] = dict(kind="random", V=2, T=48, B=8, regime="flat", W=W)
    s["ctx128_peaky_W4"] = dict(kind="random", V=128, T=48, B=8, regime="peaky", W=4)
    for W in (20, 130):
        s["c0only62_W%d" % W] = dict(kind="random", V=62, T=48, B=8, regime="peaky", W=W, table="c0only")
        s["starts62_W%d" % W] = dict(kind="random", V=62, T=48, B=8, regime="peaky", W=W, table="starts", lens=[5, 7, 9, 4, 11, 9, 14, 48])
    for src, widths in (("edge6", (4, 20, 61)), ("mix62", (20, 61))):
        for W in widths:
            V = 6 if src == "edge6" else 62
            for blank in (0, 1, V // 2, V - 1):
                s["merge_%s_b%d_W%d" % (src, blank, W)] = dict(kind="source", src=src, V=V, W=W, blank=blank)
    from ctc_pytorch_amd.testing import synth
    for boundary in (64, synth.decode_hip_constant("FAST_NTH")):
        s["chunk%d_W4" % boundary] = dict(kind="chunk", boundary=boundary, V=6, W=4)
    s["e2e62_W20"] = dict(kind="arpa", V=62, T=40, B=4, regime="peaky", W=20)
    return s


CASES = _specs()
_cache = {}


def table_for(V, kind="random", seed=77):
    """The blank-0 table of a case: context-dependent (random_table), a function of c0 alone, or the bigram table everywhere but in the
    '<s>' plane (c0 = V: the contexts of the empty and of the one-class labelling, and the final step of a one-class result)."""
    rs = np.random.RandomState(seed + V)
    if kind == "c0only":
        return with_nans(np.broadcast_to((-3.0 * rs.random_sample(V + 1))[:, None, None], (V + 1,) * 3), 0)
    if kind == "starts":
        bi = -3.0 * rs.random_sample((V + 1, V + 1))
        tri = np.array(np.broadcast_to(bi, (V + 1,) * 3))
        tri[V] = -3.0 * rs.random_sample((V + 1, V + 1))
        return with_nans(tri, 0)
    return random_table(V, seed + V)


def case(name):
    """dict(probs (T,B,V) float32, lens, tri (V+1)^3 for the case's blank, alpha, W, blank, nbest)."""
    if ("case", name) in _cache:
        return _cache[("case", name)]
    from ctc_pytorch_amd.testing import synth
    s = CASES[name]
    V, blank = s["V"], s.get("blank", 0)
    extra = {}
    if s["kind"] == "arpa":                  # a generated ARPA file with a 3-gram section, for the decoder classes: its table is the case's
        import os
        import tempfile
        from ctc_pytorch_amd.utils.NgramLM import LanguageModel
        i2c = synth.int2char(V)
        path = os.path.join(tempfile.mkdtemp(prefix="beam_trigram_"), "tg.arpa")
        synth.write_arpa(path, [i2c[i] for i in range(1, V)], seed=9, n_bigrams=600, n_trigrams=20000)
        tri = LanguageModel(path, n_gram=3).table([i2c[i] for i in range(V)])
        extra = dict(arpa=path, int2char=i2c)
    else:
        tri = table_for(V, s.get("table", "random"))
    if s["kind"] in ("random", "arpa"):
        lp = synth.make_logprobs(seed=5, T=s["T"], B=s["B"], V=V, regime=s["regime"])
        probs, lens = np.exp(lp).astype(np.float32), s.get("lens", [s["T"]] * s["B"])
    elif s["kind"] == "chunk":
        d = synth.beam_chunk_batch(s["boundary"])
        probs, lens = d["probs"], d["lens"]
    else:
        if ("sources",) not in _cache:
            import os
            from ctc_pytorch_amd.utils.NgramLM import LanguageModel
            i2c = synth.int2char(62)
            arpa = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_phone_bg.arpa")
            _cache[("sources",)] = synth.beam_sources(LanguageModel(arpa).table([i2c[i] for i in range(62)]))
        d = _cache[("sources",)][s["src"]]
        probs, lens = d["probs"], d["lens"]
    if blank:
        probs, tri, _ = move_blank3(probs, tri, blank)
    c = dict(probs=probs, lens=list(lens), tri=tri, alpha=ALPHA, W=s["W"], blank=blank, nbest=s.get("nbest", 0), **extra)
    _cache[("case", name)] = c
    return c


def reference(name):
    """decode() of the case, once per process."""
    if ("ref", name) not in _cache:
        c = case(name)
        _cache[("ref", name)] = decode(c["probs"], c["lens"], c["tri"], c["alpha"], c["W"], c["blank"], c["nbest"])
    return _cache[("ref", name)]


def compared(name):
    """The utterances of the case whose gap clears GAP: the ones a GPU result is compared on."""
    return [b for b, g in enumerate(reference(name)[3]) if g >= GAP]
