"""The inputs of tests/test_beam_edges.py, judged on the CPU against the C oracle alone (oracle/beam_ref.c, the project's authority for the
prefix beam search): they must SEPARATE the behaviours the GPU test is there to tell apart, or that test proves nothing.

The search takes three float32 decisions per frame: skip the frame when (1 - p_blank) < 0.1f; the repeat rule p_blank[t - 1] < 0.9f, t - 1
being the previous frame IN TIME; status 2 when a class of a PROCESSED frame is not > 0.  With e = float32(0.9) the first two meet: nextafter(e, 1) is
skipped, e is kept with the repeat rule false, nextafter(e, 0) is kept with the rule true.  A restatement of those rules in Python (decisions
only -- the search behind them is a plain dict-of-labellings beam) must reproduce the oracle, and each deliberately wrong variant of it must be
told from the oracle by the inputs."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import beam_ref
from ctc_pytorch_amd.testing import synth
from ctc_pytorch_amd.utils.NgramLM import LanguageModel

G = os.path.join(os.path.dirname(__file__), "golden")
WIDTHS = (4, 20, 52, 61, 130, 300)
LOG_ZERO = -99999999.0


def arpa_table62(blank=0, names=None):
    i2c = synth.int2char(62)
    return LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table(names or [i2c[i] for i in range(62)], blank)


@pytest.fixture(scope="module")
def sources():
    return synth.beam_sources(arpa_table62())


_ORACLE = {}


def oracle(src, name, W, blank=0):
    key = (name, W, blank)
    if key not in _ORACLE:
        d = src[name]
        probs, lm = d["probs"], d["lm"]
        if blank:
            probs, lm, _ = synth.move_blank(probs, lm, blank)
        ids, score, st = beam_ref.decode_ids(probs.transpose(1, 0, 2), d["lens"], lm, d["alpha"], W, blank)
        _ORACLE[key] = ([list(map(int, s)) for s in ids], np.asarray(score), [int(v) for v in st])
    return _ORACLE[key]


def differ(a, b):
    """Two (labelling, score, status) results are different results: another labelling or status, or scores more than 1e-6 relative apart."""
    return a[0] != b[0] or a[2] != b[2] or abs(a[1] - b[1]) > 1e-6 * max(abs(a[1]), abs(b[1]))


def result(o, i):
    return (o[0][i], float(o[1][i]), o[2][i])


# ---------------------------------------------------------------------------------------------------------
# the three rules, restated -- and four ways to get them wrong
# ---------------------------------------------------------------------------------------------------------
MUTANTS = ("double", "le", "prev_processed", "zero_on_skipped")


def decisions(mat, n, mutant=None):
    """Frames the search processes, each with its repeat-rule bit, and the status the log(0) rule gives (blank = class 0)."""
    e, kept, last = np.float32(0.9), [], None
    for t in range(n):
        keep = not (np.float32(1) - mat[t, 0] < np.float32(0.1))
        if not np.all(mat[t] > 0) and (keep or mutant == "zero_on_skipped"):
            return kept, 2
        if not keep:
            continue
        q = (mat[last, 0] if last is not None else None) if mutant == "prev_processed" else (mat[t - 1, 0] if t else None)
        rep = q is not None and (float(q) < 0.9 if mutant == "double" else q <= e if mutant == "le" else q < e)
        kept.append((t, bool(rep)))
        last = t
    return kept, 0


def ladd(x, y):
    if x <= LOG_ZERO:
        return y
    if y <= LOG_ZERO:
        return x
    if y - x > 0.0:
        x, y = y, x
    return x + math.log(1 + math.exp(y - x))


def search(mat, n, lm, alpha, W, mutant=None):
    """Prefix beam search over the frames `decisions` keeps (insertion-ordered dict of labellings, stable descending sort, float64 ln scores):
    (labelling, score, status), blank = class 0."""
    kept, status = decisions(mat, n, mutant)
    V = mat.shape[1]
    last = {(): [LOG_ZERO, 0.0, 0.0]}                      # labelling -> [prNonBlank, prBlank, prTotal]
    for t, rep in kept:
        lg = [math.log(float(p)) for p in mat[t]]
        curr = {}
        for y in sorted(last, key=lambda k: -last[k][2])[:W]:
            nb, _, tot = last[y]
            e = curr.setdefault(y, [LOG_ZERO, LOG_ZERO, LOG_ZERO])
            s_nb = nb + lg[y[-1]] if y else LOG_ZERO
            s_b = tot + lg[0]
            e[0], e[1], e[2] = ladd(e[0], s_nb), ladd(e[1], s_b), ladd(e[2], ladd(s_b, s_nb))
            for k in range(1, V):
                pr = lg[k] + lm[y[-1] if y else V, k] * alpha + (last[y][1] if y and y[-1] == k and rep else tot)
                x = curr.setdefault(y + (k,), [LOG_ZERO, LOG_ZERO, LOG_ZERO])
                x[0], x[2] = ladd(x[0], pr), ladd(x[2], pr)
        last = curr
    if status:
        return [], 0.0, status
    final = {}
    for y in sorted(last, key=lambda k: -last[k][2])[:W]:
        if not y:
            return [], 0.0, 1
        final[y] = (last[y][2] + lm[y[-1], V] * alpha) * (1.0 / len(y))
    best = sorted(final, key=lambda k: -final[k])[0]
    return list(best), final[best], 0


def restated(d, W, mutant=None):
    return [search(d["probs"][:, b], d["lens"][b], d["lm"], d["alpha"], W, mutant) for b in range(len(d["lens"]))]


# ---------------------------------------------------------------------------------------------------------
def test_edge_values_are_the_float32_neighbours_of_0_9():
    e, lo, hi, one, tenth = synth.BEAM_E, synth.BEAM_LO, synth.BEAM_HI, np.float32(1), np.float32(0.1)
    assert lo < e < hi and np.nextafter(lo, one) == e and np.nextafter(e, one) == hi and lo.dtype == hi.dtype == np.float32
    assert [bool(one - p < tenth) for p in (lo, e, hi)] == [False, False, True]          # skip rule
    assert [bool(p < e) for p in (lo, e, hi)] == [True, False, False]                   # repeat rule
    assert float(e) < 0.9 and float(hi) > 0.9                                           # the double constant sits between e and hi
    for p in (lo, e, hi):                                                               # 1 - p is exact, and never 0.1f itself
        assert float(one - p) == 1.0 - float(p) and one - p != tenth


CASE_SOURCES = {"edge6": WIDTHS, "status6": WIDTHS, "edge62": (4, 20, 52, 61), "status62": (4, 20, 52, 61), "mix62": WIDTHS}


def test_case_sources_run_at_the_widths_listed_here(sources):
    assert {n: tuple(sources[n]["widths"]) for n in CASE_SOURCES} == CASE_SOURCES


def kept(row):
    return not (np.float32(1) - row[0] < np.float32(0.1))


@pytest.mark.parametrize("name", sorted(CASE_SOURCES))
def test_every_case_holds_what_its_name_says_where_it_says(sources, name):
    """Read from the ARRAYS, not from the builder's word: where the edge frames and the planted values landed, whether those frames are
    kept, skipped or beyond the utterance, and which class dominates around an edge frame."""
    d = sources[name]
    A, C, Z = 2, 4, 3
    edge = {"lo": synth.BEAM_LO, "e": synth.BEAM_E, "hi": synth.BEAM_HI}
    for b, case in enumerate(d["names"]):
        p, n = d["probs"][:, b], d["lens"][b]
        dom = lambda t: int(np.argmax(np.nan_to_num(p[t, 1:], nan=-1.0))) + 1
        for t, k, v in d["plants"][b]:
            assert np.array_equal(p[t, k], v, equal_nan=True) and np.signbit(p[t, k]) == np.signbit(v), (case, t, k)
        et = [t for t, _ in d["edges"][b]]
        assert et == [t for t in range(n) if any(p[t, 0] == x for x in edge.values())], case
        for t, which in d["edges"][b]:
            assert p[t, 0] == edge[which] and kept(p[t]) == (which != "hi"), (case, t)
        tag = case.split("_")
        if case.startswith(("triple_", "t0_", "last_")):
            assert len(et) == 1 and d["edges"][b][0][1] == tag[1], case
            t = et[0]
            assert t == {"triple": t, "t0": 0, "last": n - 1}[tag[0]], case
            if tag[0] == "triple":
                assert 0 < t < n - 1 and dom(t - 1) == dom(t) == dom(t + 1) == A and kept(p[t - 1]) and kept(p[t + 1]), case
            if tag[0] == "t0":
                assert dom(0) == dom(1) == (A if d["probs"].shape[-1] == 6 else int(np.nanargmax(np.diag(d["lm"])[:-1]))) and kept(p[1]) and n > 2, case
        if case.startswith("pair_"):
            assert [w for _, w in d["edges"][b]] == tag[1:] and et[1] == et[0] + 1 and dom(et[0] - 1) == dom(et[1] + 1) == A, case
        if case.startswith("skipprev"):
            t = max(t for t in range(1, n) if kept(p[t]) and not kept(p[t - 1]))          # a kept frame behind a skipped one ...
            last = max(u for u in range(t) if kept(p[u]))
            assert p[last, 0] < edge["e"] and not p[t - 1, 0] < edge["e"] and dom(last) == dom(t) == A, case   # ... whose two readings of "previous" disagree
        plants = {(t, k): v for t, k, v in d["plants"][b]}
        bad = lambda t: not np.all(p[t] > 0)
        if case == "zero_at_t0":
            assert plants == {(0, Z): 0.0} and p[0, Z] == 0.0 and kept(p[0]) and n > 1, case
        if case == "zero_on_kept":
            assert list(plants) == [(t, Z) for t in range(n) if bad(t)] and len(plants) == 1 and all(kept(p[t]) and 0 < t < n for t, _ in plants), case
        if case in ("zero_on_skipped", "zero_on_skipped_twice"):
            assert plants and all(v == 0.0 and not kept(p[t]) and t < n for (t, _), v in plants.items()), case
            assert not any(bad(t) and kept(p[t]) for t in range(n)), case
        if case == "zero_beyond_lens":
            assert sorted(t for t, _ in plants) == [n] and p[n, Z] == 0.0 and p[n + 1, 0] == 0.0 and not any(bad(t) for t in range(n)), case
        if case == "zero_after_skipped":
            (t, k), = plants
            assert p[t, k] == 0.0 and kept(p[t]) and not kept(p[t - 1]) and t < n, case
        if case == "two_bad_frames":
            assert sorted(t for t in range(n) if bad(t) and kept(p[t])) == sorted(t for t, _ in plants) and len(plants) == 2, case
        if case in ("minus_zero", "negative", "nan_class"):
            (t, k), = plants
            assert kept(p[t]) and t < n and (np.signbit(p[t, k]) or np.isnan(p[t, k])) and not p[t, k] > 0, case
        if case == "pb_zero_on_kept":
            assert [t for t in range(n) if bad(t)] == [t for t in range(n) if p[t, 0] == 0.0] and len([t for t in range(n) if bad(t)]) == 1, case
        if case == "pb_nan":
            assert sum(np.isnan(p[t, 0]) for t in range(n)) == 1 and all(kept(p[t]) for t in range(n) if np.isnan(p[t, 0])), case
        if case == "pb_1.5":
            assert sum(p[t, 0] == np.float32(1.5) for t in range(n)) == 1 and not any(bad(t) for t in range(n)), case
        if case == "pb_one_everywhere":
            assert n == 3 and all(p[t, 0] == 1.0 for t in range(n)), case
        if case.startswith("denormal"):
            assert plants and all(0 < v < np.finfo(np.float32).tiny and kept(p[t]) and t < n for (t, _), v in plants.items()), case
    if "status" in d:
        assert d["names"].index("zero_at_t0") >= 0 and len(d["names"]) == 16
    if name.startswith("edge"):
        assert len(d["names"]) == 18


@pytest.mark.parametrize("name,W", [(n, W) for n in ("edge6", "edge62", "mix62") for W in CASE_SOURCES[n]])
def test_each_edge_triple_gives_three_different_results(sources, name, W):
    """lo / e / hi at the same frame: three pairwise different (labelling, score) results, lo and e more than 1e-6 relative apart in score.
    The cases of a group share every random mass, so the edge value alone separates them.  The one exception follows from the rules
    themselves: on an utterance's LAST frame nothing reads the repeat rule, so lo and e decode alike (the scores differ by the one ulp of
    the frame's own probabilities, far below 1e-6) and only hi (the frame is skipped) stands apart."""
    d, o = sources[name], oracle(sources, name, W)
    assert not any(o[2][i] for i, k in enumerate(d["kinds"]) if k in ("triple", "t0", "last", "pair", "skipprev"))
    groups = {"triple": ["triple_lo", "triple_e", "triple_hi"], "t0": ["t0_lo", "t0_e", "t0_hi"], "pair": ["pair_lo_lo", "pair_e_e", "pair_hi_hi"]}
    seen = 0
    for kind, names in groups.items():
        if names[0] not in d["names"]:
            continue
        lo, e, hi = (result(o, d["names"].index(n)) for n in names)
        assert differ(lo, e) and differ(e, hi) and differ(lo, hi), (kind, lo, e, hi)
        assert abs(lo[1] - e[1]) > 1e-6 * abs(e[1]), (kind, lo, e)
        seen += 1
    assert seen >= 1
    if "last_lo" in d["names"]:
        lo, e, hi = (result(o, d["names"].index(n)) for n in ("last_lo", "last_e", "last_hi"))
        assert not differ(lo, e) and differ(e, hi), (lo, e, hi)


@pytest.mark.parametrize("name,W", [(n, W) for n in ("status6", "status62") for W in CASE_SOURCES[n]])
def test_status_cases_give_the_status_the_rules_owe(sources, name, W):
    d, o = sources[name], oracle(sources, name, W)
    assert o[2] == d["status"], list(zip(d["names"], o[2], d["status"]))
    assert {0, 1, 2} == set(d["status"])
    for i, (kind, st) in enumerate(zip(d["kinds"], o[2])):
        if kind == "denormal":
            assert st == 0 and np.isfinite(o[1][i]) and o[1][i] < 0.0 and o[0][i]
        if st:
            assert o[0][i] == [] and o[1][i] == 0.0
    if name == "status62" or W > 61:
        m, o = sources["mix62"], oracle(sources, "mix62", W)
        assert len(m["status_known"]) == 6 and {n: o[2][m["names"].index(n)] for n in m["status_known"]} == m["status_known"]


@pytest.mark.parametrize("boundary", [64, synth.decode_hip_constant("FAST_NTH")])
@pytest.mark.parametrize("W", [4, 61])
def test_chunk_boundary_cases_feel_every_edge_frame(boundary, W):
    """Frames boundary - 1, boundary, boundary + 1 hold lo / e / hi in three rotations: status 0, three different results, and the rules
    restated in Python agree with the oracle while every wrong repeat rule is told apart."""
    assert boundary in (64, 1024)             # the generic kernel's p_blank load | FAST_NTH: change the GPU test's shapes with it
    d = synth.beam_chunk_batch(boundary)
    d.update(lm=-3.0 * np.random.RandomState(41).random_sample((7, 7)), alpha=0.3)
    assert d["probs"].shape == (boundary + 8, 3, 6)
    for b in range(3):
        assert sorted(d["probs"][boundary - 1:boundary + 2, b, 0]) == [synth.BEAM_LO, synth.BEAM_E, synth.BEAM_HI]
    ids, score, st = beam_ref.decode_ids(d["probs"].transpose(1, 0, 2), d["lens"], d["lm"], d["alpha"], W)
    got = [(list(map(int, ids[b])), float(score[b]), int(st[b])) for b in range(3)]
    assert not any(st) and differ(got[0], got[1]) and differ(got[1], got[2]) and differ(got[0], got[2])
    if W == 4:
        mine = restated(d, W)
        assert [(m[0], m[2]) for m in mine] == [(g[0], g[2]) for g in got]
        assert np.allclose([m[1] for m in mine], [g[1] for g in got], rtol=1e-12, atol=0)
        for mutant in ("double", "le", "prev_processed"):
            assert any(differ(m, g) for m, g in zip(restated(d, W, mutant), got)), mutant


def test_restated_rules_match_the_oracle_and_every_mutant_is_caught(sources):
    """The Python restatement reproduces the oracle on every edge and status case; each mutant -- the repeat rule against the double
    constant 0.9, with <=, against the previous PROCESSED frame; status 2 for a zero on a skipped frame -- differs from the oracle on at
    least one case of every kind that its rule touches."""
    W = 4
    touched = {"double": ("triple", "t0", "pair"), "le": ("triple", "t0", "pair"), "prev_processed": ("pair", "skipprev"),
               "zero_on_skipped": ("log0",)}
    for name in ("edge6", "status6"):
        d, o = sources[name], oracle(sources, name, W)
        want = [result(o, i) for i in range(len(d["lens"]))]
        mine = restated(d, W)
        assert [(m[0], m[2]) for m in mine] == [(w[0], w[2]) for w in want], name
        assert np.allclose([m[1] for m in mine], [w[1] for w in want], rtol=1e-12, atol=0), name
        for mutant in MUTANTS:
            mut = restated(d, W, mutant)
            for kind in touched[mutant]:
                idx = [i for i, k in enumerate(d["kinds"]) if k == kind]
                if idx:
                    assert any(differ(mut[i], want[i]) for i in idx), (mutant, kind)
    assert set(MUTANTS) == set(touched)
    # the cases the mutants fall over, by name: e is where "double" and "<=" go wrong, a skipped previous frame where "processed" does
    d, o = sources["edge6"], oracle(sources, "edge6", W)
    for mutant, case in (("double", "triple_e"), ("le", "triple_e"), ("prev_processed", "pair_hi_hi"), ("prev_processed", "skipprev_hi")):
        i = d["names"].index(case)
        assert differ(restated(d, W, mutant)[i], result(o, i)), (mutant, case)


@pytest.mark.parametrize("name", ["edge6", "status6", "edge62", "status62", "mix62", "lp9", "lp62", "ties16"])
def test_moving_the_blank_reproduces_the_blank_0_run_exactly(sources, name):
    """Class 0 moved to b in {1, V // 2, V - 1} (order of the others kept, LM permuted alike with NaN in the blank's row and column): the
    oracle's labellings mapped back, its scores bit for bit and its status words are those of the blank-0 run; no score is NaN."""
    d = sources[name]
    V = d["probs"].shape[-1]
    for W in (4, 12 if name == "lp9" else 20, 61):
        base = oracle(sources, name, W)
        assert not np.isnan(base[1]).any() and any(s == 0 for s in base[2])
        for b in (1, V // 2, V - 1):
            _, lm, old = synth.move_blank(d["probs"], d["lm"], b)
            assert np.isnan(lm[b]).all() and np.isnan(lm[:, b]).all() and old[b] == 0
            ids, score, st = oracle(sources, name, W, b)
            assert st == base[2] and [[int(old[k]) for k in s] for s in ids] == base[0], (W, b)
            assert np.array_equal(score, base[1]) and not np.isnan(score).any(), (W, b)
            assert all(b not in s for s in ids)


def test_lm_table_for_a_moved_blank_is_the_permuted_table():
    """LanguageModel.table(classes', blank_index = b) -- what BeamDecoder builds for a vocabulary whose blank sits at b -- is the blank-0 table
    with rows and columns permuted and NaN in the blank's row and column."""
    i2c, tab0 = synth.int2char(62), arpa_table62()
    assert np.isnan(tab0[0]).all() and np.isnan(tab0[:, 0]).all() and not np.isnan(tab0[1:, 1:]).any()
    for b in (1, 31, 61):
        _, want, old = synth.move_blank(np.zeros((1, 1, 62), dtype=np.float32), tab0, b)
        got = arpa_table62(b, [i2c[int(old[j])] for j in range(62)])
        assert np.array_equal(got, want, equal_nan=True), b


def test_float32_exp_of_minus_95_is_a_denormal_and_of_minus_110_is_zero():
    """The reference takes exp() of the log-probs in float32 on the host (torch.exp): -95 gives a denormal, which the search accepts
    (status 0), -110 gives 0, which it does not (status 2).  The device-side exp of the GPU test is held to the same two outcomes."""
    p = torch.exp(torch.tensor([-95.0, -110.0], dtype=torch.float32)).numpy()
    assert p.dtype == np.float32 and 0.0 < p[0] < np.finfo(np.float32).tiny and p[1] == 0.0
    d = synth.beam_exp_batch()
    probs = torch.exp(torch.from_numpy(d["lp"])).numpy()
    _, score, st = beam_ref.decode_ids(probs.transpose(1, 0, 2), d["lens"], d["lm"], d["alpha"], 4)
    assert [int(v) for v in st] == d["status"] == [0, 2, 0] and np.isfinite(score).all()
    for b, v in enumerate((-95.0, -110.0, -110.0)):
        (t, k, got), = d["plants"][b]
        assert d["lp"][t, b, k] == got == np.float32(v) and t < d["lens"][b] and kept(probs[t, b]) == (b != 2)
