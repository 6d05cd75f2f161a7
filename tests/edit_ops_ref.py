"""The restatement of the error breakdown's definition (include/ctcn.h, "Error breakdown") that tests/test_edit_ops_host.py and
tests/test_edit_ops.py compare the library with, on exact integers.

h[0..nh) is the hypothesis, r[0..nr) the reference, both after the class map.  D[i][0] = i, D[0][j] = j,
D[i][j] = min(D[i-1][j-1] + (h[i-1] != r[j-1]), D[i][j-1] + 1, D[i-1][j] + 1).  The move of (i, j) is the first of diagonal (0), deletion
(1: from (i, j-1)), insertion (2: from (i-1, j)) that attains the minimum; row 0 has only deletions, column 0 only insertions.  The alignment
is the chain of moves from (nh, nr) back to (0, 0), in forward order.

`table_literal` fills D cell by cell exactly as written above.  `table_rows` fills a row at a time for the long cases
(D[i][j] = j + min_{k <= j} (t[k] - k) with t[k] = min(diagonal, insertion) candidates of column k, t[0] = i: the deletion chain unrolled);
the host test checks that both give the same table."""
import numpy as np


def apply_map(seq, class_map):
    """ids in [0, V) are replaced by class_map[id], -1 removes the symbol; ids outside [0, V) pass through."""
    if class_map is None:
        return [int(k) for k in seq]
    V = len(class_map)
    out = []
    for k in seq:
        k = int(k)
        if 0 <= k < V:
            k = int(class_map[k])
            if k == -1:
                continue
        out.append(k)
    return out


def table_literal(h, r):
    nh, nr = len(h), len(r)
    D = np.zeros((nh + 1, nr + 1), dtype=np.int64)
    D[:, 0] = np.arange(nh + 1)
    D[0, :] = np.arange(nr + 1)
    for i in range(1, nh + 1):
        for j in range(1, nr + 1):
            D[i, j] = min(D[i - 1, j - 1] + (h[i - 1] != r[j - 1]), D[i, j - 1] + 1, D[i - 1, j] + 1)
    return D


def table_rows(h, r):
    nh, nr = len(h), len(r)
    ra = np.asarray(r, dtype=np.int64)
    D = np.zeros((nh + 1, nr + 1), dtype=np.int64)
    D[0, :] = np.arange(nr + 1)
    cols = np.arange(nr + 1)
    for i in range(1, nh + 1):
        t = np.empty(nr + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, :-1] + (ra != h[i - 1]), D[i - 1, 1:] + 1)
        D[i] = cols + np.minimum.accumulate(t - cols)
    return D


def walk(h, r, D):
    """The chain of moves of D back from (nh, nr), returned in forward order as (move, reference id or -1, hypothesis id or -1)."""
    i, j = len(h), len(r)
    ops = []
    while i > 0 or j > 0:
        if i == 0:
            m = 1
        elif j == 0:
            m = 2
        elif D[i - 1, j - 1] + (h[i - 1] != r[j - 1]) == D[i, j]:
            m = 0
        elif D[i, j - 1] + 1 == D[i, j]:
            m = 1
        else:
            m = 2
        if m == 0:
            i, j = i - 1, j - 1
            ops.append((0, r[j], h[i]))
        elif m == 1:
            j -= 1
            ops.append((1, r[j], -1))
        else:
            i -= 1
            ops.append((2, -1, h[i]))
    return ops[::-1]


def edit_ops(hyp, ref, class_map=None, table=table_literal):
    """(counts6 = [sub, del, ins, cor, nh', nr'], ops in forward order, Levenshtein distance of the mapped sequences)."""
    h, r = apply_map(hyp, class_map), apply_map(ref, class_map)
    D = table(h, r)
    ops = walk(h, r, D)
    sub = sum(1 for m, a, b in ops if m == 0 and a != b)
    cor = sum(1 for m, a, b in ops if m == 0 and a == b)
    dele = sum(1 for m, _, _ in ops if m == 1)
    ins = sum(1 for m, _, _ in ops if m == 2)
    return [sub, dele, ins, cor, len(h), len(r)], ops, int(D[len(h), len(r)])


def confusion(ops_list, V):
    """(V+1, V+1) int64: [r][h] aligned pairs, row V insertions, column V deletions; pairs with a member outside [0, V) are not entered."""
    tab = np.zeros((V + 1, V + 1), dtype=np.int64)
    inside = lambda k: 0 <= k < V
    for ops in ops_list:
        for m, a, b in ops:
            if m == 0 and inside(a) and inside(b):
                tab[a, b] += 1
            elif m == 1 and inside(a):
                tab[a, V] += 1
            elif m == 2 and inside(b):
                tab[V, b] += 1
    return tab


def batch(hyps, refs, lda, ldb, class_map=None, V=None, table=table_literal):
    """What ctcn_edit_ops answers for a batch: counts (B,6) int32, ali (B, lda+ldb, 2) int32 padded with -1, ali_len (B) int32, and the
    confusion table of the batch (None without V)."""
    B = len(hyps)
    counts = np.zeros((B, 6), dtype=np.int32)
    ali = np.full((B, lda + ldb, 2), -1, dtype=np.int32)
    ali_len = np.zeros(B, dtype=np.int32)
    all_ops = []
    for b in range(B):
        c, ops, _ = edit_ops(hyps[b], refs[b], class_map, table)
        counts[b] = c
        ali_len[b] = len(ops)
        for n, (_, a, x) in enumerate(ops):
            ali[b, n] = (a, x)
        all_ops.append(ops)
    return counts, ali, ali_len, (confusion(all_ops, V) if V is not None else None)


def small_sequences(alphabet=(0, 1, 2), max_len=4):
    """Every sequence over the alphabet of length <= max_len (121 for the defaults), shortest first."""
    out = [[]]
    last = [[]]
    for _ in range(max_len):
        last = [s + [a] for s in last for a in alphabet]
        out += last
    return out


_EXHAUSTIVE = []


def exhaustive():
    """Every (hypothesis, reference) pair of small_sequences() -- 121 x 121 = 14 641 utterances, the small alphabet forces ties -- with the
    restatement's answers (V = 3), computed once per process: (hyps, refs, counts, ali, ali_len, confusion) at lda = ldb = 4."""
    if not _EXHAUSTIVE:
        seqs = small_sequences()
        hyps = [h for h in seqs for _ in seqs]
        refs = [r for _ in seqs for r in seqs]
        _EXHAUSTIVE.append((hyps, refs) + batch(hyps, refs, 4, 4, V=3))
    return _EXHAUSTIVE[0]


def padded(seqs, width, dtype):
    """(B, width) array of the sequences, zero-filled, and their lengths."""
    out = np.zeros((len(seqs), width), dtype=dtype)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out, np.asarray([len(s) for s in seqs])
