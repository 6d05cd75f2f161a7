"""Synthetic, seed-reproducible inputs for the CTC hot path.

Imported by tests/, tools/, bench.py's input generation and oracle/gen_golden.py -- never by
the product modules of this package.  Contains no arithmetic of the path,
only NumPy ``RandomState`` data generators, so that the same tensors can be
re-created here (next to the reference) and on the GPU box (without it).

Shapes follow SURVEY.md §8(d) / BASELINE.md §3:
  x ~ N(0,1) f32 (B,T,F); labels U{2..V-1} (no blank=0 / UNK=1); lengths as the
  reference collate stores them (fractions len/Tmax in float32,
  /root/reference/timit/utils/data_loader.py:137).
"""
import math
import numpy as np

# The 61 TIMIT phones minus 'q' (the reference drops it, conf/phones.60-48-39.map:47) = 60 symbols.
TIMIT_60 = (
    "aa ae ah ao aw ax ax-h axr ay b bcl ch d dcl dh dx eh el em en eng epi er ey f g gcl "
    "h# hh hv ih ix iy jh k kcl l m n ng nx ow oy p pau pcl r s sh t tcl th uh uw ux v w y z zh"
).split()
assert len(TIMIT_60) == 60


def int2char(num_class=62):
    """index2word table as Vocab builds it (data_loader.py:16-17): 0=blank, 1=UNK, then units."""
    d = {0: "blank", 1: "UNK"}
    for i in range(2, num_class):
        d[i] = TIMIT_60[i - 2] if i - 2 < len(TIMIT_60) else "u%03d" % i
    return d


def make_batch(seed, B, T, F, V, min_len=None, lab_lo=30, lab_hi=60, full_length=False):
    """Padded utterance minibatch in the reference's input contract.

    Returns dict(x (B,T,F) f32 zero-padded, lens (B,) int, frac (B,) f32 = len/T,
    targets (B,Lmax) i64 zero-padded, tgt_len (B,) i64)."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, T, F)).astype(np.float32)
    if full_length:
        lens = np.full((B,), T, dtype=np.int64)
    else:
        lo = T // 2 if min_len is None else min_len
        lens = rs.randint(lo, T + 1, size=B).astype(np.int64)
        lens[0] = T  # one utterance defines Tmax, as in a real collate
    for b in range(B):
        x[b, lens[b]:] = 0.0
    tl = rs.randint(lab_lo, lab_hi + 1, size=B).astype(np.int64)
    # keep every sample CTC-feasible even after a /2 time stride: need T_b/2 >= L + repeats
    tl = np.minimum(tl, np.maximum(1, lens // 5))
    Lmax = int(tl.max())
    targets = np.zeros((B, Lmax), dtype=np.int64)
    for b in range(B):
        targets[b, : tl[b]] = rs.randint(2, V, size=tl[b])
    frac = np.array([np.float32(float(l) / float(T)) for l in lens], dtype=np.float32)
    return dict(x=x, lens=lens, frac=frac, targets=targets, tgt_len=tl)


def make_waves(seed, lengths, sample_rate=16000.0):
    """Waveforms for the feature front-ends: per utterance a tone of a seeded frequency (200 .. 3000 Hz, amplitude 6000) over noise of
    sigma 300, float32 on Kaldi's scale (the int16 range).  lengths: samples per utterance."""
    rs = np.random.RandomState(seed)
    out = []
    for n in lengths:
        t = np.arange(int(n)) / float(sample_rate)
        out.append((6000.0 * np.sin(2 * np.pi * rs.uniform(200.0, 3000.0) * t + rs.uniform(0, 2 * np.pi))
                    + 300.0 * rs.standard_normal(int(n))).astype(np.float32))
    return out


def fill_state_dict(shapes, seed):
    """Deterministic parameter values for a CTC_Model state_dict.

    ``shapes``: ordered list of (key, shape).  RNN/Linear/Conv weights ~ U(-b,b) with
    b = 1/sqrt(fan), BN gamma ~ 1+0.1N, beta ~ 0.1N,
    running_mean=0, running_var=1, num_batches_tracked=0."""
    rs = np.random.RandomState(seed)
    out = {}
    for key, shape in shapes:
        shape = tuple(shape)
        leaf = key.split(".")[-1]
        if leaf == "num_batches_tracked":
            out[key] = np.zeros((), dtype=np.int64)
        elif leaf == "running_mean":
            out[key] = np.zeros(shape, dtype=np.float32)
        elif leaf == "running_var":
            out[key] = np.ones(shape, dtype=np.float32)
        elif "batch_norm" in key or key.startswith("fc.0."):
            if leaf == "weight":
                out[key] = (1.0 + 0.1 * rs.standard_normal(shape)).astype(np.float32)
            else:
                out[key] = (0.1 * rs.standard_normal(shape)).astype(np.float32)
        else:
            if len(shape) == 1:
                fan = shape[0]
            elif len(shape) == 2:
                fan = shape[1]
            else:
                fan = int(np.prod(shape[1:]))
            b = 1.0 / math.sqrt(max(fan, 1))
            out[key] = rs.uniform(-b, b, size=shape).astype(np.float32)
    return out


def write_arpa(path, units, seed=7, n_bigrams=600, n_trigrams=0):
    """Synthetic phone bigram LM in the exact text format NgramLM.initngrams parses
    (/root/reference/timit/utils/NgramLM.py:38-56): header lines ``\\1-grams:`` /
    ``\\2-grams:``, TAB-separated ``log10prob<TAB>token[<TAB>log10backoff]``.
    n_trigrams > 0: every bigram that can open a trigram (its second token is not ``</s>``) gets a back-off weight and a
    ``\\3-grams:`` section of that many entries follows; about a third of them extend a pair that is NO bigram entry (back-off
    through an absent bigram), and ``<s>`` only ever stands first.  The trigram draws come from a stream of their own, so the
    unigram and bigram lines are the ones n_trigrams = 0 writes, but for the added back-off column."""
    rs = np.random.RandomState(seed)
    rs3 = np.random.RandomState(seed + 1000003)
    toks = ["<s>", "</s>", "<unk>"] + list(units)
    lines = ["", "\\data\\", "ngram 1=%d" % len(toks), "ngram 2=%d" % n_bigrams]
    if n_trigrams:
        lines.append("ngram 3=%d" % n_trigrams)
    lines += ["", "\\1-grams:"]
    for t in toks:
        p = -3.0 * rs.random_sample()
        if t == "</s>":
            lines.append("%.6f\t%s" % (p, t))
        else:
            bo = -1.0 * rs.random_sample()
            lines.append("%.6f\t%s\t%.6f" % (p, t, bo))
    lines += ["", "\\2-grams:"]
    seen = set()
    firsts = [t for t in toks if t != "</s>"]
    seconds = [t for t in toks if t != "<s>"]
    while len(seen) < n_bigrams:
        a = firsts[rs.randint(len(firsts))]
        b = seconds[rs.randint(len(seconds))]
        if (a, b) in seen:
            continue
        seen.add((a, b))
        if n_trigrams and b != "</s>":
            lines.append("%.6f\t%s %s\t%.6f" % (-3.0 * rs.random_sample(), a, b, -1.0 * rs3.random_sample()))
        else:
            lines.append("%.6f\t%s %s" % (-3.0 * rs.random_sample(), a, b))
    if n_trigrams:
        lines += ["", "\\3-grams:"]
        heads = sorted(ab for ab in seen if ab[1] != "</s>")
        mids = [t for t in toks if t not in ("<s>", "</s>")]
        seen3 = set()
        while len(seen3) < n_trigrams:
            if rs3.random_sample() < 2.0 / 3.0:
                a, b = heads[rs3.randint(len(heads))]
            else:
                a, b = firsts[rs3.randint(len(firsts))], mids[rs3.randint(len(mids))]
            c = seconds[rs3.randint(len(seconds))]
            if (a, b, c) in seen3:
                continue
            seen3.add((a, b, c))
            lines.append("%.6f\t%s %s %s" % (-3.0 * rs3.random_sample(), a, b, c))
    lines += ["", "\\end\\", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def _log_softmax(z):
    z = z.astype(np.float64)
    m = z.max(axis=-1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))).astype(np.float32)


def make_logits(seed, T, B, V, regime="peaky", blank_frac=0.6):
    """(T,B,V) f32 *logits* for decoder tests.
    peaky: 8*onehot(random CTC path with ~60 % blank frames) + N(0,1); flat: 3*N(0,1)."""
    rs = np.random.RandomState(seed)
    if regime == "flat":
        return (3.0 * rs.standard_normal((T, B, V))).astype(np.float32)
    z = rs.standard_normal((T, B, V)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            if rs.random_sample() < blank_frac:
                k, run = 0, rs.randint(1, 6)
            else:
                k, run = rs.randint(2, V), rs.randint(1, 4)
            z[t : t + run, b, k] += 8.0
            t += run
    return z


def make_logprobs(seed, T, B, V, regime="peaky"):
    return _log_softmax(make_logits(seed, T, B, V, regime))


# ---------------------------------------------------------------------------------------------------------
# Beam search: inputs that sit ON the search's float32 decisions, and a blank that is not class 0
# (tests/test_beam_edges.py on the GPU and tests/test_beam_edges_host.py on the CPU judge the same arrays).
# Everything is a float32 PROBABILITY built with the blank at class 0; move_blank() re-homes it.
# ---------------------------------------------------------------------------------------------------------
BEAM_E = np.float32(0.9)                                  # skip rule and repeat rule meet here in float32
BEAM_LO = np.nextafter(BEAM_E, np.float32(0))             # kept, repeat rule true
BEAM_HI = np.nextafter(BEAM_E, np.float32(1))             # skipped (1 - p exact: 0.099999964 < 0.1f), repeat rule false
BEAM_EDGE = {"lo": BEAM_LO, "e": BEAM_E, "hi": BEAM_HI}
_A, _C, _Z = 2, 4, 3                                      # two dominant classes and the class that carries a planted value


def decode_hip_constant(name):
    """An integer `constexpr int NAME = value` of csrc/decode.hip (the fast kernel's FAST_NTH: frames per compaction pass)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "decode.hip")
    with open(path) as f:
        m = re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*[^,;]+,\s*)*?%s\s*=\s*(\d+)" % re.escape(name), f.read())
    assert m, name
    return int(m.group(1))


def beam_frame(rs, V, pb, dom):
    """One frame, blank = class 0 with probability `pb` (taken as it is: 1.5 and NaN included); the other classes share 1 - pb in
    float32 (0.1 where pb is no probability below 1), class `dom` about two thirds of it, the rest small random mass."""
    pb = np.float32(pb)
    w = (rs.uniform(0.2, 0.8, size=V) / V).astype(np.float32)
    w[dom] = np.float32(1.0)
    w[0] = np.float32(0.0)
    mass = np.float32(1) - pb if np.float32(0) <= pb < np.float32(1) else np.float32(0.1)
    row = (w / w.sum(dtype=np.float32) * mass).astype(np.float32)
    row[0] = pb
    return row


def _low_blank(n, V, step, off=0):
    """n frames with p_blank = 1e-4 and changing dominant classes.  A few of them in an utterance and the EMPTY labelling leaves a beam of
    any width up to 300, so the utterance ends with status 0 unless its case says otherwise."""
    return [(1e-4, 1 + (step * t + off) % (V - 1)) for t in range(n)]


def _beam_cases(cases, V, seed, T=None):
    """cases: list of (name, kind, frames, beyond).  `frames` are ALL frames of the utterance, in order, `beyond` the frames right behind its
    end; a frame is (p_blank, dominant class) or (p_blank, dominant class, {class: planted value}).  Nothing is shifted or added here: frame
    t of the list is frame t of the array.  Frames further out are ordinary kept frames: a search that reads them changes its result.
    Returns probs (T, B, V), lens, names, kinds and, for the tests to check where things landed, plants[b] = [(t, class, value)] and
    edges[b] = [(t, 'lo' | 'e' | 'hi')]."""
    import zlib
    B = len(cases)
    T = T or max(len(c[2]) + len(c[3]) for c in cases) + 1
    probs = np.zeros((T, B, V), dtype=np.float32)
    lens, plants, edges = [], [], []
    for b, (_, kind, frames, beyond) in enumerate(cases):
        # the cases of one kind draw the SAME small random masses: what tells lo, e and hi apart is the edge value alone
        rs = np.random.RandomState((seed + zlib.crc32(kind.encode())) % (1 << 31))
        listed = list(frames) + list(beyond)
        plants.append([])
        edges.append([])
        for t in range(T):
            f = listed[t] if t < len(listed) else (0.25, 1 + (t + len(frames)) % (V - 1))
            probs[t, b] = beam_frame(rs, V, f[0], f[1])
            for k, v in (f[2] if len(f) > 2 else {}).items():
                probs[t, b, k] = np.float32(v)
                plants[b].append((t, k, np.float32(v)))
            for n, x in BEAM_EDGE.items():
                if np.float32(f[0]) == x:
                    edges[b].append((t, n))
        lens.append(len(frames))
    return dict(probs=probs, lens=lens, names=[c[0] for c in cases], kinds=[c[1] for c in cases], plants=plants, edges=edges)


def beam_edge_batch(V=6, seed=11, pre=5, post=3, t0_class=_A):
    """The repeat / skip edge at every position (kinds 'triple', 't0', 'last', 'pair', 'skipprev').  N = an ordinary kept frame; every case
    is run-in frames + its own frames + run-out frames, except that a 't0' case starts with its edge frame and a 'last' case ends with it.
    `t0_class`: the dominant class of the first two frames of the 't0' cases -- one whose repetition the LM table in use makes likely, or
    no labelling with that class doubled can win."""
    N = lambda k: (0.25, k)
    front, back, long_back = _low_blank(pre, V, 3), _low_blank(post, V, 2, 1), _low_blank(pre + post, V, 2, 1)
    cases = []
    for n, x in BEAM_EDGE.items():
        cases.append(("triple_" + n, "triple", front + [N(_A), (x, _A), N(_A), N(_C)] + back, []))
    for n, x in BEAM_EDGE.items():
        # (class a of the edge frame holds 3.0 -- no probability, the search takes it as it is --, or the empty labelling's 0.9 would feed
        # "a" so much that no labelling with the doubled a, the one the repeat rule decides about, could win)
        cases.append(("t0_" + n, "t0", [(x, t0_class, {t0_class: 3.0}), (1e-4, t0_class), N(_C)] + long_back, []))
    for n, x in BEAM_EDGE.items():
        cases.append(("last_" + n, "last", front + [N(_A), N(_C), (x, _C)], []))
    for n, m in (("lo", "lo"), ("e", "e"), ("hi", "hi"), ("lo", "hi"), ("hi", "lo"), ("e", "lo")):
        cases.append(("pair_%s_%s" % (n, m), "pair", front + [N(_A), (BEAM_EDGE[n], _A), (BEAM_EDGE[m], _A), N(_A), N(_C)] + back, []))
    # the previous frame IN TIME is skipped (repeat rule false), the previous PROCESSED frame has p_blank = 0.25 (it would say true)
    cases.append(("skipprev_hi", "skipprev", front + [N(_A), (BEAM_HI, _C), N(_A), N(_C)] + back, []))
    cases.append(("skipprev_0.97", "skipprev", front + [N(_C), N(_A), (0.97, _A), N(_A)] + back, []))
    cases.append(("skipprev_two", "skipprev", front + [N(_A), (BEAM_HI, _C), (1.0, _C), N(_A), N(_A)] + back, []))
    return _beam_cases(cases, V, seed)


def beam_status_batch(V=6, seed=12, pre=5, post=3):
    """Blank values that are no probability, the log(0) rule at every place it can apply, denormals.  `status`: what the search owes
    (0 ok, 1 empty labelling at the end, 2 log of a value that is not > 0) -- the host test holds the C restatement of the search to it.
    N = an ordinary kept frame, S = a skipped one, P(k, v) = a kept frame with the value v planted in class _Z."""
    N = lambda k: (0.25, k)
    S = lambda k, plant=None: (0.97, k, plant or {})
    P = lambda k, v, cls=_Z: (0.25, k, {cls: v})
    front, back, long_back = _low_blank(pre, V, 3), _low_blank(post, V, 2, 1), _low_blank(pre + post, V, 2, 1)
    tiny = np.float32(1e-40)
    least = np.nextafter(np.float32(0), np.float32(1))                         # 2^-149
    assert 0 < least < tiny < np.finfo(np.float32).tiny
    cases = [
        ("pb_one_everywhere", "allskipped", [(1.0, _A), (1.0, _C), (1.0, _A)], [], 1),
        ("pb_1.5", "blankval", front + [N(_A), (1.5, _C), N(_A)] + back, [], 0),
        ("pb_nan", "blankval", front + [N(_A), (np.nan, _C), N(_A)] + back, [], 2),
        ("zero_on_skipped", "log0", front + [N(_A), S(_C, {_Z: 0.0}), N(_A)] + back, [], 0),
        ("zero_on_kept", "log0", front + [N(_A), P(_C, 0.0), N(_A)] + back, [], 2),
        ("zero_at_t0", "log0_t0", [P(_A, 0.0), N(_C)] + long_back, [], 2),                     # frame 0 itself, kept
        ("zero_beyond_lens", "log0", front + [N(_A), N(_C)] + back, [P(_A, 0.0), (0.0, _C)], 0),
        ("pb_zero_on_kept", "log0", front + [N(_A), (0.0, _C), N(_A)] + back, [], 2),
        ("minus_zero", "log0", front + [N(_A), P(_C, -0.0), N(_A)] + back, [], 2),
        ("negative", "log0", front + [N(_A), N(_C), P(_A, -0.25)] + back, [], 2),
        ("nan_class", "log0", front + [N(_A), P(_C, np.nan), N(_A)] + back, [], 2),
        ("zero_after_skipped", "log0", front + [N(_A), S(_C), P(_C, 0.0)] + back, [], 2),
        ("zero_on_skipped_twice", "log0", front + [S(_A, {_Z: 0.0}), N(_A), S(_C, {_A: 0.0}), N(_C)] + back, [], 0),
        ("two_bad_frames", "log0", front + [N(_A), P(_C, 0.0), N(_A), P(_C, np.nan, _A)] + back, [], 2),
        ("denormal_1e-40", "denormal", front + [N(_A), P(_C, tiny), N(_A)] + back, [], 0),
        ("denormal_least", "denormal", front + [N(_A), P(_C, least), P(_A, tiny, 1)] + back, [], 0),
    ]
    d = _beam_cases([c[:4] for c in cases], V, seed)
    d["status"] = [c[4] for c in cases]
    return d


def beam_chunk_batch(boundary, seed=13, V=6):
    """Three long utterances with edge frames at boundary - 1, boundary, boundary + 1 (the values rotated over the utterances, so every
    position sees lo, e and hi), one class dominant around them so that the repeat rule decides; T = boundary + 8.  One frame in three
    is skipped elsewhere, so the list of processed frames does not run in step with time."""
    T = boundary + 8
    vals = [BEAM_LO, BEAM_E, BEAM_HI]
    cases = []
    for b in range(3):
        frames = []
        for t in range(T):
            near = abs(t - boundary) <= 3
            if boundary - 1 <= t <= boundary + 1:
                frames.append((vals[(b + t - boundary + 1) % 3], _A))
            elif near:
                frames.append((0.25, _A))
            elif t % 3 == 1:
                frames.append((0.97, 1 + t % (V - 1)))
            else:
                frames.append((0.25, 1 + (t // 3) % (V - 1)))
        cases.append(("chunk%d_%d" % (boundary, b), "chunk", frames, []))
    return _beam_cases(cases, V, seed, T=T)


def move_blank(probs, lm, b):
    """Re-home the blank from class 0 to class b, keeping the order of the other classes: returns (probs', lm', old) with old[j] = the
    class that now sits at j.  The LM table is permuted alike (row and column V stay last) and gets NaN in row b and column b."""
    V = probs.shape[-1]
    old = np.array([c for c in range(1, b + 1)] + [0] + [c for c in range(b + 1, V)], dtype=np.int64)
    assert sorted(old) == list(range(V)) and old[b] == 0
    ext = np.concatenate([old, [V]])
    lm2 = np.array(lm, dtype=np.float64)[np.ix_(ext, ext)]
    lm2[b, :] = np.nan
    lm2[:, b] = np.nan
    return np.ascontiguousarray(probs[..., old]), lm2, old


def _take(d, names):
    idx = [d["names"].index(n) for n in names]
    out = dict(probs=np.ascontiguousarray(d["probs"][:, idx]), names=list(names))
    for key in ("lens", "kinds", "plants", "edges", "status"):
        if key in d:
            out[key] = [d[key][i] for i in idx]
    return out


def beam_sources(arpa_table62):
    """Every batch the beam-edge tests decode: name -> dict(probs (T,B,V) float32, lens, lm (V+1,V+1) float64 for blank 0, alpha,
    widths: the beam widths it runs at; names / kinds / plants / edges / status where the batch is made of cases; lp: the log-probs a
    random batch was made from).  `arpa_table62`: the golden ARPA bigram table for int2char(62), blank 0."""
    src = {}
    every = [4, 20, 52, 61, 130, 300]
    for name, V, seed in (("edge6", 6, 21), ("status6", 6, 22)):
        d = beam_edge_batch(V) if name == "edge6" else beam_status_batch(V)
        lm = -3.0 * np.random.RandomState(seed).random_sample((V + 1, V + 1))
        lm[_A, _A] = 0.0                # (a after a costs nothing: the labelling with the doubled a can win where the repeat rule allows it)
        d.update(lm=lm, alpha=0.3, widths=every)
        src[name] = d
    # The same cases at the model's alphabet with the golden LM, a shorter run-in.  The checker's time grows with W^2 V: all of them run up to
    # W = 61 (edge62, status62), ten of them -- one of every kind of decision -- at every width (mix62).
    arpa = np.array(arpa_table62, dtype=np.float64)
    likeliest_repeat = int(np.nanargmax(np.diag(arpa)[:62]))
    e, s = beam_edge_batch(62, pre=2, post=1, t0_class=likeliest_repeat), beam_status_batch(62, pre=2, post=1)
    src["edge62"] = dict(e, lm=arpa, alpha=0.1, widths=[4, 20, 52, 61])
    src["status62"] = dict(s, lm=arpa, alpha=0.1, widths=[4, 20, 52, 61])
    e = _take(e, ["triple_lo", "triple_e", "triple_hi", "skipprev_hi"])
    s = _take(s, ["pb_nan", "zero_on_skipped", "zero_on_kept", "zero_at_t0", "zero_beyond_lens", "denormal_1e-40"])
    T = max(e["probs"].shape[0], s["probs"].shape[0])
    pad = lambda p: np.concatenate([p, np.full((T - p.shape[0],) + p.shape[1:], np.float32(1.0 / 62), dtype=np.float32)])
    mix = {k: e[k] + s[k] for k in ("lens", "names", "kinds", "plants", "edges")}
    mix.update(probs=np.concatenate([pad(e["probs"]), pad(s["probs"])], axis=1), status_known={n: st for n, st in zip(s["names"], s["status"])},
               lm=arpa, alpha=0.1, widths=every)
    src["mix62"] = mix
    for name, V, W, seed in (("lp9", 9, 12, 31), ("lp62", 62, 20, 32)):
        lp = make_logprobs(seed=seed, T=40, B=6, V=V, regime="peaky")
        lm = np.array(arpa_table62, dtype=np.float64) if V == 62 else -3.0 * np.random.RandomState(seed).random_sample((V + 1, V + 1))
        src[name] = dict(lp=lp, probs=np.exp(lp).astype(np.float32), lens=[0, 1, 40, 23, 31, 40], lm=lm, alpha=0.1 if V == 62 else 0.3, widths=sorted(set(every + [W])))
    T, B, V = 14, 6, 16            # every class 1 / V on every frame: all extensions tie to the last bit
    src["ties16"] = dict(probs=np.full((T, B, V), 1.0 / V, dtype=np.float32), lens=[T, T - 1, 1, 0, T // 2, T], lm=np.zeros((V + 1, V + 1)), alpha=0.0,
                         widths=every)
    return src


def beam_exp_batch(V=6, seed=14, pre=5):
    """LOG-probs for the searches' own float32 exp: -95 in one class of a kept frame (exp is a denormal: status 0), -110 there (exp is 0:
    status 2), -110 on a skipped frame (never looked at: status 0).  plants[b] = [(t, class, log-prob)]."""
    N = lambda k: (0.25, k)
    front, back = _low_blank(pre, V, 3), _low_blank(3, V, 2, 1)
    d = _beam_cases([("exp_-95", "exp", front + [N(_A), N(_C), N(_A)] + back, []), ("exp_-110", "exp", front + [N(_A), N(_C), N(_A)] + back, []),
                     ("exp_-110_skipped", "exp", front + [N(_A), (0.97, _C), N(_A)] + back, [])], V, seed)
    lp = np.log(d["probs"]).astype(np.float32)
    t = len(front) + 1
    for b, v in enumerate((-95.0, -110.0, -110.0)):
        lp[t, b, _Z] = np.float32(v)
        d["plants"][b] = [(t, _Z, np.float32(v))]
    d.update(lp=lp, status=[0, 2, 0], lm=-3.0 * np.random.RandomState(seed).random_sample((V + 1, V + 1)), alpha=0.3)
    del d["probs"]
    return d
