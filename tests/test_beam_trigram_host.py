"""Trigram LM scoring of the beam search, everything that needs no GPU: LanguageModel(n_gram=3) against a dict lookup written here, the
Python restatement (tests/beam_trigram_ref.py) against the C oracle under a context-free table, the order-3 plan, the refusals, and the
gap rule that the GPU tests of tests/test_beam_trigram.py lean on."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import beam_trigram_ref as R
from oracle import beam_ref
from ctc_pytorch_amd.testing import synth

G = os.path.join(os.path.dirname(__file__), "golden")
GENERIC_STATIC_LDS = {256: 176, 512: 448, 1024: 1376}
BEAM_OPTIONS = {"beam_fast": 1, "beam_occ2": 0, "beam_generic_threads": 0, "beam_cand_global": 0}
LN10 = math.log(10)


# ---- LanguageModel(n_gram=3) --------------------------------------------------------------------------------------------------------
def read_arpa(path):
    """{order: {tokens: (log10 p, log10 back-off)}} by a parser of this file's own."""
    out, cur = {}, None
    with open(path) as f:
        for line in f.read().split("\n"):
            if line.startswith("\\") and line.endswith("-grams:"):
                cur = out.setdefault(int(line[1]), {})
            elif line.startswith("\\"):
                cur = None
            elif cur is not None and line:
                p = line.split("\t")
                cur[tuple(p[1].split(" "))] = (float(p[0]), float(p[2]) if len(p) > 2 else 0.0)
    return out


def lookup_bi(g, a, b):
    if (a, b) in g[2]:
        return LN10 * g[2][(a, b)][0]
    return LN10 * g[1][(a,)][1] + LN10 * g[1][(b,)][0]


def lookup_tri(g, a, b, c):
    if (a, b, c) in g[3]:
        return LN10 * g[3][(a, b, c)][0]
    return (LN10 * g[2][(a, b)][1] if (a, b) in g[2] else 0.0) + lookup_bi(g, b, c)


@pytest.fixture(scope="module")
def arpa3(tmp_path_factory):
    d = tmp_path_factory.mktemp("lm3")
    units = [synth.int2char(13)[i] for i in range(2, 13)]         # (not class 1, 'UNK': the parser aliases it to '<unk>')
    p3, p2 = str(d / "tg.arpa"), str(d / "bg.arpa")
    synth.write_arpa(p3, units, seed=9, n_bigrams=60, n_trigrams=400)
    synth.write_arpa(p2, units, seed=9, n_bigrams=60)
    return p3, p2, units


def test_write_arpa_default_bytes_and_the_added_section(arpa3, tmp_path):
    """n_trigrams = 0 writes what it wrote before the argument existed (golden digest of the default file); with trigrams the unigram
    and bigram probabilities are the same lines plus a back-off column."""
    import hashlib
    p3, p2, units = arpa3
    g3, g2 = read_arpa(p3), read_arpa(p2)
    assert 3 not in g2 and len(g3[3]) == 400 and g3[1] == g2[1] and set(g3[2]) == set(g2[2])
    assert all(g3[2][k][0] == g2[2][k][0] for k in g2[2]) and any(v[1] != 0.0 for v in g3[2].values())
    assert all("<s>" not in k[1:] and "</s>" not in k[:2] for k in g3[3])
    q = str(tmp_path / "default.arpa")
    synth.write_arpa(q, [synth.int2char(62)[i] for i in range(1, 62)])
    with open(os.path.join(G, "beam_trigram.json")) as f:
        assert hashlib.sha256(open(q, "rb").read()).hexdigest() == json.load(f)["write_arpa_default_sha256"]


def test_get_tri_prob_is_the_arpa_back_off(arpa3):
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    p3, _, units = arpa3
    lm, g = LanguageModel(p3, n_gram=3), read_arpa(p3)
    assert len(lm.trigrame) == 400 and all(len(k.split(" ")) == 2 for k in lm.bigram)
    toks = ["<s>"] + units + ["<unk>"]
    seen = {"hit": 0, "bo_present": 0, "bo_absent": 0, "start": 0, "end": 0, "start2": 0}
    for a in toks:
        for b in toks[1:]:
            for c in toks[1:] + ["</s>"]:
                want = lookup_tri(g, a, b, c)
                got = lm.get_tri_prob("" if a == "<s>" else a, b, "" if c == "</s>" else c)
                assert got == want, (a, b, c)
                seen["hit" if (a, b, c) in g[3] else "bo_present" if (a, b) in g[2] else "bo_absent"] += 1
                seen["start"] += a == "<s>"
                seen["end"] += c == "</s>"
    for c in toks[1:]:
        assert lm.get_tri_prob("", "", c) == lookup_tri(g, "<s>", "<s>", c)
        seen["start2"] += 1
    assert all(v > 0 for v in seen.values()), seen
    s = "%s %s %s" % (units[0], units[3], units[3])
    want = lookup_bi(g, "<s>", units[0]) + lookup_tri(g, "<s>", units[0], units[3]) + lookup_tri(g, units[0], units[3], units[3]) + \
        lookup_tri(g, units[3], units[3], "</s>")
    assert abs(lm.score_tg(s) - want) <= 4 * np.spacing(abs(want))
    with pytest.raises(KeyError):
        lm.get_tri_prob(units[0], "nophone", units[1])


@pytest.mark.parametrize("blank", [0, 5, 11])
def test_table3_values_and_nan_pattern(arpa3, blank):
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    p3, _, units = arpa3
    lm, g = LanguageModel(p3, n_gram=3), read_arpa(p3)
    V = 12
    classes = {c: "" for c in range(V)}
    for c, u in zip([c for c in range(V) if c != blank], units):
        classes[c] = u
    classes[blank] = "_"
    tab = lm.table(classes, blank)
    assert tab.shape == (V + 1,) * 3 and tab.dtype == np.float64
    tok = lambda c, end: (("</s>" if end else "<s>") if c == V else classes[c])
    for c0 in range(V + 1):
        for c1 in range(V + 1):
            for k in range(V + 1):
                dead = blank in (c0, c1, k) or (c1 == V and c0 != V)
                if dead:
                    assert np.isnan(tab[c0, c1, k]), (c0, c1, k)
                elif c0 == V and c1 == V:
                    assert tab[c0, c1, k] == lookup_bi(g, "<s>", tok(k, True)) == lm.get_bi_prob("", "" if k == V else classes[k])
                else:
                    assert tab[c0, c1, k] == lookup_tri(g, tok(c0, False), tok(c1, False), tok(k, True)), (c0, c1, k)


def test_n_gram_2_ignores_the_section_in_its_table(arpa3):
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    p3, p2, units = arpa3
    classes = ["_"] + units
    a, b = LanguageModel(p3).table(classes), LanguageModel(p2).table(classes)
    assert a.shape == (13, 13) and np.array_equal(a, b, equal_nan=True)
    assert not hasattr(LanguageModel(p3), "trigrame")
    assert LanguageModel(p3, n_gram=3).get_bi_prob(units[0], units[1]) == LanguageModel(p2).get_bi_prob(units[0], units[1])


def test_decoder_classes_pass_the_order_on(arpa3):
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    from ctc_pytorch_amd.steps import decode_ctc
    p3, _, units = arpa3
    classes = ["_"] + units
    d3, d2 = BeamDecoder(classes, 5, lm_path=p3, lm_alpha=0.3, lm_order=3), BeamDecoder(classes, 5, lm_path=p3, lm_alpha=0.3)
    assert d3._decoder.lm.n_gram == 3 and d3._decoder._lm_table().shape == (13, 13, 13)
    assert d2._decoder.lm.n_gram == 2 and d2._decoder._lm_table().shape == (13, 13)
    a = decode_ctc.arg_parser().parse_args(["--conf", "x", "--lm-order", "3"])
    assert decode_ctc.apply_argv({}, a) == {"lm_order": 3}
    assert "lm_order" not in decode_ctc.apply_argv({}, decode_ctc.arg_parser().parse_args(["--conf", "x"]))

    class Opts(object):
        decode_type, beam_width, lm_path, lm_alpha = "Beam", 5, p3, 0.3
    assert decode_ctc.lm_order_option(Opts) == 2 and decode_ctc.make_decoder(Opts, classes)._decoder.lm.n_gram == 2
    Opts.lm_order = 3
    assert decode_ctc.make_decoder(Opts, classes)._decoder.lm.n_gram == 3
    Opts.lm_order = 4
    with pytest.raises(ValueError):
        decode_ctc.lm_order_option(Opts)


# ---- the restatement against the C oracle ------------------------------------------------------------------------------------------
def test_restatement_equals_the_c_oracle_on_the_golden_decoder_sets():
    """Bigram table and context-free 3-D table: labellings, status and scores bit-equal, 1-best and n-best, every golden beam set."""
    z = np.load(os.path.join(G, "decoders.npz"))
    meta = json.load(open(os.path.join(G, "decoders.json")))
    i2c = synth.int2char(62)
    tab = beam_ref.arpa_table(os.path.join(G, "lm_phone_bg.arpa"), i2c)
    tri = R.context_free(tab)
    n = 0
    for key, want_strings in meta.items():
        if not key.startswith("beam_"):
            continue
        _, regime, w, a = key.split("_")
        W, alpha = int(w[1:]), float(a[1:])
        probs = np.exp(z["lp_" + regime].astype(np.float32))
        want = beam_ref.decode_ids(np.ascontiguousarray(probs.transpose(1, 0, 2)), meta["lens"], tab, alpha, W)
        for table in (tab, tri):
            got = R.decode(probs, meta["lens"], table, alpha, W)
            assert got[0] == [list(map(int, s)) for s in want[0]] and got[2] == list(want[2]) and np.array_equal(got[1], want[1]), key
        assert [" ".join(i2c[k] for k in s) for s in got[0]] == want_strings
        N = min(W, 3)
        wn = beam_ref.decode_ids_nbest(np.ascontiguousarray(probs.transpose(1, 0, 2)), meta["lens"], tab, alpha, W, N)
        gn = R.decode(probs, meta["lens"], tri, alpha, W, nbest=N)
        assert gn[0] == wn[0] and np.array_equal(gn[1], wn[1]) and gn[2] == list(wn[2]), key
        n += 1
    assert n >= 10


@pytest.mark.parametrize("name", ["edge6", "status6", "mix62", "ties16"])
def test_restatement_equals_the_c_oracle_at_the_edges(name):
    """... and on the edge, status and tie batches of the beam-edge tests (merges, repeats, status 1 and 2), blank 0 and moved."""
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    i2c = synth.int2char(62)
    d = synth.beam_sources(LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(62)]))[name]
    V = d["probs"].shape[-1]
    for blank in (0, V // 2):
        probs, lm, _ = synth.move_blank(d["probs"], d["lm"], blank) if blank else (d["probs"], d["lm"], None)
        for W in (4, 20):
            want = beam_ref.decode_ids_nbest(np.ascontiguousarray(probs.transpose(1, 0, 2)), d["lens"], lm, d["alpha"], W, 3, blank)
            got = R.decode(probs, d["lens"], R.context_free(lm), d["alpha"], W, blank, nbest=3)
            assert got[0] == want[0] and got[2] == list(want[2]) and np.array_equal(got[1], want[1]), (name, blank, W)


def test_a_context_dependent_table_changes_the_labellings():
    """The order-3 term is live: most labellings of the two regimes change against the context-free table of the same bigrams."""
    changed = 0
    for regime in ("peaky", "flat"):
        c = R.case("ctx62_%s_W20" % regime)
        a = R.decode(c["probs"], c["lens"], c["tri"], 0.5, 20)
        b = R.decode(c["probs"], c["lens"], R.with_nans(R.context_free(c["tri"][62]), 0), 0.5, 20)
        changed += sum(x != y for x, y in zip(a[0], b[0]))
    assert changed >= 8


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def options():
    from ctc_pytorch_amd import ops
    yield ops.set_option
    for k, v in BEAM_OPTIONS.items():
        ops.set_option(k, v)


def test_order_3_fits_one_workgroup_at_the_widest_beam(options):
    """W = 1 024, V = 62: the beam state with one class more per slot, plus the kernel's static LDS, within 160 KB; the table stays in
    global memory; 8 KB (2 x 1 024 ints) more than order 2."""
    from ctc_pytorch_amd import ops
    p3 = ops.beam_plan(24, 2, 62, 1024, 160 * 1024, GENERIC_STATIC_LDS[1024], lm_order=3)
    p2 = ops.beam_plan(24, 2, 62, 1024, 160 * 1024, GENERIC_STATIC_LDS[1024])
    assert p3["rc"] == 0 and p3["path"] == 2 and p3["generic_fits"] == 1 and p3["lm_in_lds"] == 0 and p3["threads"] == 1024
    assert GENERIC_STATIC_LDS[1024] + p3["generic_lds"] <= 160 * 1024
    assert p3["generic_lds"] - p2["generic_lds"] == 2 * 1024 * 4
    assert ops.beam_plan(24, 2, 62, 1024, 64 * 1024, GENERIC_STATIC_LDS[1024], lm_order=3)["rc"] == -3


def test_order_2_through_the_new_diagnostic_is_the_old_answer(options):
    from ctc_pytorch_amd import _lib
    L = _lib.lib()
    a, b = (ctypes.c_int * 19)(), (ctypes.c_int * 19)()
    pa, pb = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)
    n = 0
    for occ2 in (0, 1, 2):
        options("beam_occ2", occ2)
        for fast in (1, 0):
            options("beam_fast", fast)
            for V in (3, 6, 62, 128, 257):
                for W in (1, 20, 60, 61, 200, 1024):
                    for lds_max in (65536, 163840):
                        assert L.ctcn_diag_beam_plan(800, 4, V, W, lds_max, 1376, pa) == L.ctcn_diag_beam_plan_lm(800, 4, V, W, 2, lds_max, 1376, pb)
                        assert list(a) == list(b), (occ2, fast, V, W, lds_max)
                        n += 1
    assert n == 360


def test_order_3_plan_rule_on_a_grid(options):
    """Restated from the kernels' contracts: the order-3 table is never in LDS; the fast kernel takes the shapes it takes at order 2
    (W <= 60, at most 4 candidates per thread, its LDS within 144 KB -- 67 KB for the occ2 builds, whose order-3 static LDS is 768 B
    larger) and gives the trie the room the table would have had; the generic kernel's plan is the order-2 plan without the LM table
    and with 2 ints more per beam slot."""
    from ctc_pytorch_amd import ops
    fast = 0
    for occ2 in (0, 1, 2):
        options("beam_occ2", occ2)
        for V in (2, 6, 62, 128):
            for W in (1, 4, 20, 52, 60, 61, 130, 300, 1024):
                for T in (48, 1032):
                    options("beam_fast", 1)
                    p3 = ops.beam_plan(T, 8, V, W, lm_order=3, generic_static_lds=1376)
                    npt = -(-W * V // 832)
                    core = (W * V + 2 * V) * 8 + (W * V + T) * 4
                    budget = (67 if occ2 else 144) * 1024
                    slots = 16384
                    while slots > 1024 and core + slots * 4 > budget:
                        slots >>= 1
                    ok = W <= 60 and npt <= 4 and core + slots * 4 <= budget
                    assert (p3["ok"], p3["lm_lds"], p3["lm_in_lds"], p3["rc"]) == (int(ok), 0, 0, 0), (occ2, V, W, T)
                    assert p3["path"] == ((1 if occ2 else 0) if ok else 2), (occ2, V, W, T)
                    if ok:
                        assert (p3["npt"], p3["trie_slots"], p3["lds"]) == (npt, slots, core + slots * 4), (occ2, V, W, T)
                    fast += ok
                    options("beam_fast", 0)
                    g3, g2 = ops.beam_plan(T, 8, V, W, lm_order=3, generic_static_lds=1376), ops.beam_plan(T, 8, V, W, generic_static_lds=1376)
                    assert g3["path"] == 2 and g3["lm_in_lds"] == 0 and g3["rc"] == 0
                    assert all(g3[k] == g2[k] for k in ("threads", "wcap", "smax", "ws_generic", "ws_fast", "max_nodes", "ht_size")), (V, W)
                    wcap, smax = g3["wcap"], g3["smax"]
                    base = V * 8 + wcap * (10 * 8 + 12 * 4) + smax * 12
                    cand_in = 1376 + base + 256 + W * V * 8 <= 160 * 1024
                    assert (g3["cand_in_lds"], g3["generic_lds"]) == (int(cand_in), base + (W * V * 8 if cand_in else 0)), (V, W)
    assert fast > 50


def test_refusals_touch_no_device(options):
    """Bad arguments, another order and a table over the 64-MiB cap: refused by the diagnostic and, before any HIP call, by the decode
    entry (dummy non-null pointers: a call that got past the checks would fault); a 3-D table of the wrong shape never leaves Python."""
    import torch
    from ctc_pytorch_amd import _lib, ops
    L = _lib.lib()
    out = (ctypes.c_int * 19)()
    o = ctypes.cast(out, ctypes.c_void_p)
    assert L.ctcn_diag_beam_plan_lm(70, 2, 62, 20, 3, 163840, 176, o) == 0
    assert L.ctcn_diag_beam_plan_lm(70, 2, 128, 4, 3, 163840, 176, o) == 0                  # 129^3 doubles = 17 MB
    assert L.ctcn_diag_beam_plan_lm(70, 2, 202, 4, 3, 163840, 176, o) == 0                  # 203^3 doubles: the last V under 64 MiB
    assert 203 ** 3 * 8 <= 64 << 20 < 204 ** 3 * 8
    for bad in ((0, 2, 62, 20, 3, 163840, 176), (70, 2, 1, 20, 3, 163840, 176), (70, 2, 62, 1025, 3, 163840, 176), (70, 2, 62, 20, 3, 0, 176)):
        assert L.ctcn_diag_beam_plan_lm(*bad, o) == -1, bad
    assert L.ctcn_diag_beam_plan_lm(70, 2, 62, 20, 3, 163840, 176, None) == -1
    for order, V in ((1, 62), (4, 62), (0, 62), (3, 203), (3, 1000)):
        assert L.ctcn_diag_beam_plan_lm(70, 2, V, 20, order, 163840, 176, o) == -3, (order, V)
        assert ops.beam_plan(70, 2, V, 20, lm_order=order)["rc"] == -3
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for order, V in ((4, 62), (3, 203)):
        rc = L.ctcn_beam_decode_lm(p, 1, p, p, order, 0.5, 4, 0, 1, p, p, p, None, p, 3, 1, V, p, 1 << 20, None)
        assert rc == -3 and b"order" in L.ctcn_last_error(), (order, V)
    assert L.ctcn_beam_decode_lm(p, 1, p, p, 3, 0.5, 4, 0, 5, p, p, p, None, p, 3, 1, 6, p, 1 << 20, None) == -1      # nbest > W
    x = torch.zeros(5, 2, 6)
    for shape in ((7, 7, 6), (6, 7, 7), (8, 8, 8), (1, 7, 7)):
        for call in (lambda t: ops.beam_decode(x, [5, 5], t, 0.5, 4), lambda t: ops.beam_decode_nbest(x, [5, 5], t, 0.5, 4, 2),
                     lambda t: ops.beam_decode_async(x, [5, 5], t, 0.5, 4), lambda t: ops.beam_decode_device(x, [5, 5], t, 0.5, 4)):
            with pytest.raises(ValueError):
                call(np.zeros(shape))


# ---- the gap rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_every_compared_utterance_clears_the_gap(name):
    """What tests/test_beam_trigram.py compares with the restatement: every cut and every neighbour pair of the final sort at least 1e-9
    apart (relative) -- the GPU's scores are held to 4 spacings, ~1e-15 -- in all utterances but at most one in ten per batch, and
    the batch is no row of status words."""
    c = R.case(name)
    want = R.reference(name)
    keep = R.compared(name)
    B = len(c["lens"])
    assert (want[3][keep] >= R.GAP).all() and 10 * (B - len(keep)) <= B, (name, want[3])
    assert any(want[2][b] == 0 for b in keep), (name, want[2])
