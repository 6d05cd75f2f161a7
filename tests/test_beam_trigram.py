"""Trigram LM scoring in the beam search (csrc/decode.hip, order 3) on every search path the library can be put on -- the configurations
tests/test_beam_edges.py enumerates for a width: the fast kernel and its two occ2 builds, the generic kernel by threads x candidate
placement x selection -- against the Python restatement tests/beam_trigram_ref.py, which tests/test_beam_trigram_host.py holds to the C
oracle bit for bit under a context-free table.

A context-free 3-D table must give the order-2 call's bits.  Under a context-dependent table labellings and status equal the
restatement's and scores lie within the suite's 4 spacings on every utterance whose decisions are at least 1e-9 (relative) apart in the
restatement (R.compared; the host file asserts that this leaves out at most one utterance in ten); all paths of a width agree bit for
bit on every utterance."""
import os

import numpy as np
import pytest
import torch

import beam_trigram_ref as R
from test_beam_edges import DEFAULTS, FAST, GENERIC, paths
from ctc_pytorch_amd.testing import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def run(x, lens, lm, alpha, W, blank, opts, nbest=0):
    """One search with the options of `opts` set and every beam option back at its default afterwards; the order is the table's rank."""
    from ctc_pytorch_amd import ops
    T, B, V = x.shape
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        if opts.get("beam_fast", 1) == 1 and W <= 60 and W * V <= 4 * 832:       # (W = 60 at V = 62: five candidates per thread, the generic kernel)
            want_path = 1 if opts.get("beam_occ2", 0) else 0
            assert ops.beam_plan(T, B, V, W, lm_order=np.ndim(lm))["path"] == want_path, "this case was meant for the fast kernel"
        if nbest:
            ids, score, st = ops.beam_decode_nbest(x, lens, lm, alpha, W, nbest, blank, input_is_prob=True)
        else:
            ids, score, st = ops.beam_decode(x, lens, lm, alpha, W, blank, input_is_prob=True)
    finally:
        for k, v in DEFAULTS.items():
            ops.set_option(k, v)
    return ids, np.asarray(score), [int(v) for v in st]


def bit_equal(a, b, what):
    assert a[0] == b[0] and a[2] == b[2], what
    assert np.array_equal(a[1], b[1]), (what, [(i, float(u), float(v)) for i, (u, v) in enumerate(zip(np.ravel(a[1]), np.ravel(b[1]))) if u != v])


def same_as_restatement(got, want, keep, what):
    """On the compared utterances: labellings and status equal, scores within 4 spacings and never NaN; a status other than 0 returns no
    labelling and score 0."""
    assert not np.isnan(got[1]).any(), what
    for b in keep:
        assert got[2][b] == want[2][b], (what, b, got[2], want[2])
        assert got[0][b] == want[0][b], (what, b)
        assert np.all(np.abs(got[1][b] - want[1][b]) <= 4 * np.spacing(np.abs(want[1][b]))), (what, b, got[1][b], want[1][b])
        if got[2][b]:
            assert not got[0][b] and not np.any(got[1][b]), (what, b)


def every_path(dev, name, configs=None):
    """The case on every configuration of its width: each equals the restatement on the compared utterances and the first one bit for bit."""
    c, want, keep = R.case(name), R.reference(name), R.compared(name)
    x = torch.from_numpy(c["probs"]).to(dev)
    first = None
    for cname, opts in (configs or paths(c["W"])):
        got = run(x, c["lens"], c["tri"], c["alpha"], c["W"], c["blank"], opts, c["nbest"])
        same_as_restatement(got, want, keep, (name, cname))
        if first is None:
            first = got
        bit_equal(got, first, (name, cname))
    assert all(c["blank"] not in s for s in first[0]) or c["nbest"]
    return first


# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 20, 60, 61, 130, 300])
def test_context_free_table_gives_the_order_2_bits(dev, W):
    """tri[c0] = the bigram table for every c0: ids, status and scores of the order-3 call equal the order-2 call's on every path --
    random batches of both regimes with the golden ARPA table, and the edge / status mix (non-zero status words) with a moved blank."""
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    i2c = synth.int2char(62)
    arpa = LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(62)])
    batches = [(np.exp(synth.make_logprobs(seed=5, T=48, B=8, V=62, regime=r)).astype(np.float32), [48, 47, 1, 0, 30, 48, 48, 12], arpa, 0.5, 0)
               for r in ("peaky", "flat")]
    mix = synth.beam_sources(arpa)["mix62"]
    for blank in (0, 31):
        probs, lm, _ = synth.move_blank(mix["probs"], mix["lm"], blank) if blank else (mix["probs"], mix["lm"], None)
        batches.append((probs, mix["lens"], lm, mix["alpha"], blank))
    for n, (probs, lens, lm, alpha, blank) in enumerate(batches):
        x, tri = torch.from_numpy(probs).to(dev), R.with_nans(R.context_free(lm), blank)
        for cname, opts in paths(W):
            two, three = run(x, lens, lm, alpha, W, blank, opts), run(x, lens, tri, alpha, W, blank, opts)
            bit_equal(three, two, (n, W, cname))
            bit_equal(run(x, lens, tri, alpha, W, blank, opts, nbest=min(W, 3)), run(x, lens, lm, alpha, W, blank, opts, nbest=min(W, 3)), (n, W, cname, "nbest"))
        assert n >= 2 or any(st == 0 and s for st, s in zip(two[2], two[0]))
    assert any(two[2])                                   # (the mix: status words other than 0 travel alike)


CTX = [n for n in R.CASES if n.startswith("ctx")]


@pytest.mark.parametrize("name", CTX)
def test_context_dependent_table_on_every_path(dev, name):
    """Random back-offs, a third of the entries explicit, alpha = 0.5: V = 62 (peaky and flat) at W = 1 ... 300 and once at W = 1 024,
    V = 6, V = 2, V = 128."""
    # (W = 1 024: every forced thread count is raised to 1 024 threads, so the default one stands for all four)
    first = every_path(dev, name, GENERIC[:4] if R.CASES[name]["W"] > 512 else None)
    assert any(st == 0 and len(s) >= 2 for st, s in zip(first[2], first[0]))


def test_the_first_index_is_live_at_v_128(dev):
    """V = 128, the 17-MB table: the scores differ from those under the context-free table of its '<s>' plane."""
    c = R.case("ctx128_peaky_W4")
    x = torch.from_numpy(c["probs"]).to(dev)
    a = run(x, c["lens"], c["tri"], c["alpha"], 4, 0, FAST[0][1])
    b = run(x, c["lens"], R.with_nans(R.context_free(c["tri"][128]), 0), c["alpha"], 4, 0, FAST[0][1])
    assert a[2] == b[2] == [0] * 8 and not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith(("c0only", "starts"))])
def test_context_plumbing_one_fault_per_table(dev, name):
    """A table that depends on c0 alone (a wrong class-before-last shows in the score and nowhere else), and one whose '<s>' plane alone
    differs from a bigram table (the contexts of the empty and the one-class labelling, the final step of a one-class result: utterances
    of 1 ... 9 frames are in the batch)."""
    first = every_path(dev, name)
    if name.startswith("starts"):
        assert any(st == 0 and len(s) == 1 for st, s in zip(first[2], first[0])), "no one-class result in the batch"
    assert sum(st == 0 for st in first[2]) >= 4


@pytest.mark.parametrize("src,W", [("edge6", 4), ("edge6", 20), ("edge6", 61), ("mix62", 20), ("mix62", 61)])
def test_merges_and_repeats_with_a_moved_blank(dev, src, W):
    """The edge6 / mix62 batches (stays that merge with their parent's extension, repeats at the float32 edges) under a context-dependent
    table, blank at 0, 1, V // 2 and V - 1 (a 3-D move_blank: NaN in the blank's planes): every path equals the restatement, and the
    moved-blank runs mapped back are the blank-0 run bit for bit."""
    V = 6 if src == "edge6" else 62
    base = None
    for blank in (0, 1, V // 2, V - 1):
        name = "merge_%s_b%d_W%d" % (src, blank, W)
        first = every_path(dev, name)
        old = R.blank_order(V, blank)
        back = ([[int(old[k]) for k in s] for s in first[0]], first[1], first[2])
        if blank == 0:
            base = back
        else:
            bit_equal(back, base, (name, "moved blank against blank 0"))
    assert any(st == 0 for st in base[2])


@pytest.mark.parametrize("boundary", [64, synth.decode_hip_constant("FAST_NTH")])
def test_across_the_chunk_boundaries(dev, boundary):
    """T = boundary + 8 across the generic kernel's 64-frame p_blank load and the fast kernel's FAST_NTH-frame compaction; V = 6, W = 4 on
    every fast and generic configuration."""
    first = every_path(dev, "chunk%d_W4" % boundary, FAST + GENERIC)
    assert first[2] == [0, 0, 0] and len({float(s) for s in first[1]}) == 3


@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith("nbest")])
def test_nbest(dev, name):
    """nbest = 3 at W = 20 and W = 130 on every path; entry 0 is what beam_decode returns."""
    c = R.case(name)
    first = every_path(dev, name)
    assert all(len(u) == 3 for u in first[0])
    x = torch.from_numpy(c["probs"]).to(dev)
    one = run(x, c["lens"], c["tri"], c["alpha"], c["W"], 0, paths(c["W"])[0][1])
    assert [u[0] for u in first[0]] == one[0] and np.array_equal(first[1][:, 0], one[1]) and first[2] == one[2]


def test_decoder_classes_end_to_end(dev):
    """BeamDecoder(lm_order=3) on a generated ARPA file with a 3-gram section: decode, decode_async, decode_timed and decode_nbest return
    the restatement's strings (its table is LanguageModel(n_gram=3).table); with lm_order = 2 the same file decodes as its bigrams."""
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    name = "e2e62_W20"
    c, want, keep = R.case(name), R.reference(name), R.compared(name)
    i2c = c["int2char"]
    assert len(keep) == len(c["lens"]) and want[2] == [0] * len(keep)
    strings = [" ".join(i2c[k] for k in s) for s in want[0]]
    bd = BeamDecoder(i2c, beam_width=c["W"], blank_index=0, space_idx=-1, lm_path=c["arpa"], lm_alpha=c["alpha"], lm_order=3)
    lp = torch.log(torch.from_numpy(c["probs"]))
    assert bd._decoder.decode(torch.from_numpy(c["probs"]).transpose(0, 1), c["lens"]) == strings
    base = bd.decode(lp, c["lens"])
    assert bd.decode_async(lp, c["lens"])() == base and all(base)
    timed = bd.decode_timed(lp, c["lens"])
    assert bd.timed_strings(timed) == base
    nb, score = bd._decoder.decode_nbest(torch.from_numpy(c["probs"]).transpose(0, 1), c["lens"], 3)
    wn = R.decode(c["probs"], c["lens"], c["tri"], c["alpha"], c["W"], 0, nbest=3)
    assert [u[0] for u in nb] == strings and np.all(np.abs(score[:, 0] - want[1]) <= 4 * np.spacing(np.abs(want[1])))
    if (wn[3] >= R.GAP).all():
        assert nb == [[" ".join(i2c[k] for k in s) for s in u] for u in wn[0]]
    two = BeamDecoder(i2c, beam_width=c["W"], blank_index=0, space_idx=-1, lm_path=c["arpa"], lm_alpha=c["alpha"])
    want2 = R.decode(c["probs"], c["lens"], two._decoder._lm_table(), c["alpha"], c["W"])
    assert two._decoder.decode(torch.from_numpy(c["probs"]).transpose(0, 1), c["lens"]) == [" ".join(i2c[k] for k in s) for s in want2[0]]
    assert want2[0] != want[0]
