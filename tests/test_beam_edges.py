"""The beam search (csrc/decode.hip) at its decision edges and with a blank that is not class 0, on every search path the library can be
put on, against the C oracle (oracle/beam_ref.c) called with the same blank.

decode.hip restates three float32 decisions in three families of kernel (beam_prep_kernel + the fast kernel and its occ2 builds; the generic
kernel at 256 / 512 / 1 024 threads, candidates in LDS or global memory, bitonic or rank-count selection; the n-best entry): skip a frame
when (1 - p_blank) < 0.1f, the repeat rule p_blank[t - 1] < 0.9f on the previous frame IN TIME, status 2 for a class of a PROCESSED frame that
is not > 0.  The inputs (ctc_pytorch_amd/testing/synth.py, judged on the CPU by tests/test_beam_edges_host.py) put p_blank on float32(0.9)
and its two neighbours -- where both compares flip -- at t = 0, at the last frame, twice in a row, behind a skipped frame and across the
64-frame p_blank load of the generic kernel and the FAST_NTH-frame compaction pass of the fast one; plant 0, -0.0, negative, NaN and denormal
values on kept, skipped and out-of-length frames; and move the blank to classes 1, V // 2 and V - 1 with NaN in the blank's row and column of
the LM table, so that a read of it shows in the score."""
import os

import numpy as np
import pytest
import torch

from oracle import beam_ref
from ctc_pytorch_amd.testing import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
WIDTHS = (4, 20, 52, 61, 130, 300)
# source -> the widths it runs at.  All edge and status cases at V = 62 run up to W = 61, ten of them (mix62: one of every kind of decision) at
# every width: the C oracle's time grows with W^2 V.
SOURCES = {"edge6": WIDTHS, "status6": WIDTHS, "edge62": WIDTHS[:4], "status62": WIDTHS[:4], "mix62": WIDTHS, "lp9": (4, 12, 20, 52, 61, 130, 300),
           "lp62": WIDTHS, "ties16": WIDTHS}
DEFAULTS = {"beam_fast": 1, "beam_occ2": 0, "beam_generic_threads": 0, "beam_cand_global": 0, "beam_bitonic": 1}
GENERIC = [("generic_t%d_g%d_b%d" % (t, g, s), {"beam_fast": 0, "beam_generic_threads": t, "beam_cand_global": g, "beam_bitonic": s})
           for t in (0, 256, 512, 1024) for g in (0, 1) for s in (0, 1)]
FAST = [("fast_occ%d" % o, {"beam_fast": 1, "beam_occ2": o}) for o in (0, 1, 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def arpa_table62():
    from ctc_pytorch_amd.utils.NgramLM import LanguageModel
    i2c = synth.int2char(62)
    return LanguageModel(os.path.join(G, "lm_phone_bg.arpa")).table([i2c[i] for i in range(62)])


@pytest.fixture(scope="module")
def sources():
    return synth.beam_sources(arpa_table62())


def paths(W):
    """Every configuration a search of width W can run in: the fast kernel and its occ2 builds plus the generic kernel (beam_fast = 0) up to
    W = 60, the generic kernel's thread counts x candidate placements x selections beyond."""
    return FAST + [("generic", {"beam_fast": 0})] if W <= 60 else GENERIC


def run(x, lens, lm, alpha, W, blank, opts, is_prob=True, nbest=0):
    """One search with the options of `opts` set and every beam option back at its default afterwards."""
    from ctc_pytorch_amd import ops
    T, B, V = x.shape
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        if opts.get("beam_fast", 1) == 1 and W <= 60:       # (the library's own plan under these options: 0 / 1 = the fast kernel / its occ2 build)
            assert ops.beam_plan(T, B, V, W)["path"] == (1 if opts.get("beam_occ2", 0) else 0), "this case was meant for the fast kernel"
        if nbest:
            ids, score, st = ops.beam_decode_nbest(x, lens, lm, alpha, W, nbest, blank, input_is_prob=is_prob)
        else:
            ids, score, st = ops.beam_decode(x, lens, lm, alpha, W, blank, input_is_prob=is_prob)
    finally:
        for k, v in DEFAULTS.items():
            ops.set_option(k, v)
    return ids, np.asarray(score), [int(v) for v in st]


_ORACLE = {}


def oracle(key, probs, lens, lm, alpha, W, blank, nbest=0):
    """The C oracle once per (batch, width, blank, nbest), whichever test asks first."""
    key = key + (W, blank, nbest)
    if key not in _ORACLE:
        p = np.ascontiguousarray(probs.transpose(1, 0, 2))
        if nbest:
            ids, score, st = beam_ref.decode_ids_nbest(p, lens, lm, alpha, W, nbest, blank)
        else:
            ids, score, st = beam_ref.decode_ids(p, lens, lm, alpha, W, blank)
            ids = [list(map(int, s)) for s in ids]
        _ORACLE[key] = (ids, np.asarray(score), [int(v) for v in st])
    return _ORACLE[key]


def same_as_oracle(got, want, what):
    """Labellings and status words equal, float64 scores within the suite's gate of 4 spacings (ocml's exp / log against glibc's); an
    utterance whose status is not 0 returns what the oracle returns -- no labelling, score 0 (spacing(0) admits nothing else)."""
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[0] == want[0], what
    assert got[1].shape == want[1].shape and not np.isnan(got[1]).any(), what
    assert np.all(np.abs(got[1] - want[1]) <= 4 * np.spacing(np.abs(want[1]))), (what, got[1], want[1])
    for b, st in enumerate(got[2]):
        if st:
            assert not got[0][b] and not np.any(got[1][b]), (what, b)


def bit_equal(a, b, what):
    assert a[0] == b[0] and a[2] == b[2], what
    assert np.array_equal(a[1], b[1]), (what, [(i, float(u), float(v)) for i, (u, v) in enumerate(zip(np.ravel(a[1]), np.ravel(b[1]))) if u != v])


def mapped_back(got, old):
    relabel = lambda s: [relabel(u) for u in s] if s and isinstance(s[0], list) else [int(old[k]) for k in s]
    return [relabel(s) for s in got[0]], got[1], got[2]


def all_paths_all_blanks(dev, key, d, W, configs, blanks):
    """The heart of this file: for blank 0 and every moved blank, every configuration equals the oracle called with that blank and,
    bit for bit, the first configuration; the moved-blank run mapped back equals the blank-0 run of the same kernels bit for bit."""
    V = d["probs"].shape[-1]
    base = None
    for blank in blanks:
        probs, lm, old = synth.move_blank(d["probs"], d["lm"], blank) if blank else (d["probs"], d["lm"], np.arange(V))
        want = oracle(key, probs, d["lens"], lm, d["alpha"], W, blank)
        if "status" in d:
            assert want[2] == d["status"]
        for n, st in d.get("status_known", {}).items():
            assert want[2][d["names"].index(n)] == st
        x = torch.from_numpy(probs).to(dev)
        first = None
        for name, opts in configs:
            got = run(x, d["lens"], lm, d["alpha"], W, blank, opts)
            same_as_oracle(got, want, (key, W, blank, name))
            if first is None:
                first = got
            bit_equal(got, first, (key, W, blank, name))
        assert all(blank not in s for s in first[0])
        if blank == 0:
            base = first
        else:
            bit_equal(mapped_back(first, old), base, (key, W, blank, "moved blank against blank 0"))
    return base


# ---------------------------------------------------------------------------------------------------------
def test_no_beam_option_is_left_out():
    """The configurations above are built from these five options: a sixth that the library learns must join them."""
    from ctc_pytorch_amd import ops
    assert sorted(n for n in ops.option_names() if n.startswith("beam")) == sorted(DEFAULTS)
    assert {k: ops.get_option(k) for k in DEFAULTS} == DEFAULTS


@pytest.mark.parametrize("name,W", [(n, W) for n in SOURCES for W in SOURCES[n]])
def test_every_path_at_the_edges_and_with_a_moved_blank(dev, sources, name, W):
    """Edge, status and denormal cases at V = 6 and V = 62, two random batches (lengths 0, 1 and T among them) and the uniform tie batch: every
    search path of width W, blank at 0, 1, V // 2 and V - 1."""
    d = sources[name]
    V = d["probs"].shape[-1]
    assert tuple(d["widths"]) == SOURCES[name]
    if "status_known" in d:
        assert len(d["status_known"]) == 6
    base = all_paths_all_blanks(dev, (name,), d, W, paths(W), (0, 1, V // 2, V - 1))
    assert any(st == 0 for st in base[2])
    for kind, st, score in zip(d.get("kinds", []), base[2], base[1]):
        if kind == "denormal":
            assert st == 0 and np.isfinite(score) and score < 0.0


@pytest.mark.parametrize("boundary", [64, synth.decode_hip_constant("FAST_NTH")])
def test_edge_frames_across_the_chunk_boundaries(dev, boundary):
    """lo / e / hi on frames boundary - 1, boundary, boundary + 1 of utterances boundary + 8 frames long: 64 = the frames per p_blank load of
    the generic kernel, which carries the previous frame's value across loads; FAST_NTH = the frames per compaction pass of the fast
    kernel's frame list.  W = 4 on every fast and generic configuration (beam_fast = 0 sends W = 4 to the generic kernel), W = 61 on the
    generic ones; blank 0 and V // 2."""
    d = synth.beam_chunk_batch(boundary)
    d.update(lm=-3.0 * np.random.RandomState(41).random_sample((7, 7)), alpha=0.3)
    assert d["probs"].shape == (boundary + 8, 3, 6) and d["lens"] == [boundary + 8] * 3
    for W, configs in ((4, FAST + GENERIC), (61, GENERIC)):
        base = all_paths_all_blanks(dev, ("chunk", boundary), d, W, configs, (0, 3))
        assert base[2] == [0, 0, 0] and len({float(s) for s in base[1]}) == 3


NBEST = [(20, FAST[0]), (61, GENERIC[3])]


def nbest_all_blanks(dev, key, d, W, config, blanks, log_input=False):
    """ctcn_beam_decode_nbest, nbest = 3, in one configuration: the oracle's n-best lists with the same blank, entry 0 = what beam_decode
    returns on the same path, the moved-blank run mapped back = the blank-0 run bit for bit.  log_input: the batch holds log-probs (d["lp"]),
    the kernel takes the exp and the oracle gets the float32 exp of the host."""
    V, N = d["lm"].shape[0] - 1, min(W, 3)
    base = None
    for blank in blanks:
        if log_input:
            _, lm, old = synth.move_blank(d["lp"], d["lm"], blank) if blank else (None, d["lm"], np.arange(V))
            lp = np.ascontiguousarray(d["lp"][..., old])
            probs, x = torch.exp(torch.from_numpy(lp)).numpy(), torch.from_numpy(lp).to(dev)
        else:
            probs, lm, old = synth.move_blank(d["probs"], d["lm"], blank) if blank else (d["probs"], d["lm"], np.arange(V))
            x = torch.from_numpy(probs).to(dev)
        want = oracle(key, probs, d["lens"], lm, d["alpha"], W, blank, N)
        got = run(x, d["lens"], lm, d["alpha"], W, blank, config[1], is_prob=not log_input, nbest=N)
        if log_input:           # (the two exps may differ in the last bit: status and labellings, as for the 1-best searches)
            assert got[2] == want[2] == d["status"] and got[0] == want[0] and np.isfinite(got[1]).all(), (key, W, blank)
        else:
            same_as_oracle(got, want, (key, W, blank))
        one = run(x, d["lens"], lm, d["alpha"], W, blank, config[1], is_prob=not log_input)
        assert [u[0] if u else [] for u in got[0]] == one[0] and np.array_equal(got[1][:, 0], one[1]) and got[2] == one[2], (key, W, blank)
        if blank == 0:
            base = got
        else:
            bit_equal(mapped_back(got, old), base, (key, W, blank))
    return base


@pytest.mark.parametrize("name", sorted(SOURCES))
@pytest.mark.parametrize("W,config", NBEST)
def test_nbest_at_the_edges_and_with_a_moved_blank(dev, sources, name, W, config):
    """The n-best entry (its own final sort and LM end term in both kernels) on every batch of this file, the fast kernel at W = 20 and the
    generic one at W = 61, blank at 0, 1, V // 2 and V - 1."""
    d = sources[name]
    V = d["probs"].shape[-1]
    base = nbest_all_blanks(dev, (name,), d, W, config, (0, 1, V // 2, V - 1))
    assert any(len(u) == 3 for u in base[0])


@pytest.mark.parametrize("boundary", [64, synth.decode_hip_constant("FAST_NTH")])
def test_nbest_across_the_chunk_boundaries_and_through_the_device_exp(dev, boundary):
    """The chunk-boundary batch of `boundary` through the n-best entry (the fast kernel at W = 4 and 20, the generic one at W = 4 and 61),
    and with it the -95 / -110 log-prob batch through the n-best entry's device-side exp; blank at 0, 1, V // 2 and V - 1."""
    d = synth.beam_chunk_batch(boundary)
    d.update(lm=-3.0 * np.random.RandomState(41).random_sample((7, 7)), alpha=0.3)
    for W, config in ((4, FAST[0]), (4, ("generic", {"beam_fast": 0}))) + tuple(NBEST):
        base = nbest_all_blanks(dev, ("chunk", boundary), d, W, config, (0, 1, 3, 5))
        assert base[2] == [0, 0, 0] and all(len(u) == 3 for u in base[0])
    e = synth.beam_exp_batch()
    for W, config in ((4, FAST[0]), (4, ("generic", {"beam_fast": 0}))) + tuple(NBEST):
        nbest_all_blanks(dev, ("exp",), e, W, config, (0, 1, 3, 5), log_input=True)


@pytest.mark.parametrize("name", ["lp9", "lp62", "ties16", "status6", "status62"])
def test_device_side_exp_with_a_moved_blank(dev, sources, name):
    """input_is_prob = False (beam_prep_kernel's expf on the fast path, the generic kernel's own): status and labellings equal the run on
    probabilities, blank at 0, 1, V // 2, V - 1 -- on batches whose outcome does not hang on the last bit of expf: random soft-maxes, the
    uniform batch (equal inputs give equal outputs whatever that bit is) and the status cases (log(0) = -inf and log of a negative value =
    NaN come back as 0 and NaN, a denormal stays far from 0, 0.97 and 1.5 far from 0.9).  The lo / e / hi batches are left out on purpose:
    exp(log(x)) need not return x, two correct float32 exps may land on different sides of 0.9, and the reference defines the result only
    for its own host exp."""
    d = sources[name]
    V = d["probs"].shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        lp0 = d["lp"] if "lp" in d else np.log(d["probs"]).astype(np.float32)
    for blank in (0, 1, V // 2, V - 1):
        probs, lm, old = synth.move_blank(d["probs"], d["lm"], blank) if blank else (d["probs"], d["lm"], np.arange(V))
        x, lp = torch.from_numpy(probs).to(dev), torch.from_numpy(np.ascontiguousarray(lp0[..., old])).to(dev)
        for W, config in ((20, FAST[0]), (20, ("generic", {"beam_fast": 0})), (61, GENERIC[0])):
            want = run(x, d["lens"], lm, d["alpha"], W, blank, config[1])
            got = run(lp, d["lens"], lm, d["alpha"], W, blank, config[1], is_prob=False)
            assert got[2] == want[2] and got[0] == want[0] and not np.isnan(got[1]).any(), (name, blank, W, config[0])


def test_device_side_exp_keeps_a_denormal_and_rejects_a_zero(dev):
    """Log-probs of -95 and -110 in one class of a kept frame: float32 exp gives a denormal (status 0, finite score) and 0 (status 2), as
    torch.exp does on the host (tests/test_beam_edges_host.py); -110 on a skipped frame is never looked at.  Fast path (beam_prep_kernel)
    in its three builds, generic kernel at W = 4 and W = 61; blank 0 and V // 2."""
    d = synth.beam_exp_batch()
    V = d["lp"].shape[-1]
    for blank in (0, V // 2):
        _, lm, old = synth.move_blank(d["lp"], d["lm"], blank) if blank else (None, d["lm"], np.arange(V))
        lp = np.ascontiguousarray(d["lp"][..., old])
        probs = torch.exp(torch.from_numpy(lp)).numpy()                   # the reference's arithmetic: float32 exp on the host
        x = torch.from_numpy(lp).to(dev)
        for W, configs in ((4, FAST + [("generic", {"beam_fast": 0})]), (61, GENERIC[:1])):
            want = oracle(("exp",), probs, d["lens"], lm, d["alpha"], W, blank)
            assert want[2] == d["status"] == [0, 2, 0]
            for cname, opts in configs:
                got = run(x, d["lens"], lm, d["alpha"], W, blank, opts, is_prob=False)
                assert got[2] == want[2] and got[0] == want[0], (blank, W, cname, got[2])
                assert np.isfinite(got[1]).all() and got[1][0] < 0.0 and got[1][1] == 0.0, (blank, W, cname)


def test_decoder_classes_with_a_moved_blank(dev, sources):
    """BeamDecoder(int2char', blank_index = b) with the permuted vocabulary and the golden ARPA file -- the LM table comes from
    LanguageModel.table(classes, blank_index) -- returns the strings of the blank-0 decoder; ctcBeamSearch.decode, the entry that takes
    probabilities, returns the oracle's strings; a zero on a kept frame raises ValueError at blank b as at blank 0."""
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    i2c, arpa, W = synth.int2char(62), os.path.join(G, "lm_phone_bg.arpa"), 20
    for name in ("lp62", "mix62"):
        d = sources[name]
        want = oracle((name,), d["probs"], d["lens"], d["lm"], d["alpha"], W, 0)
        ok = [b for b, st in enumerate(want[2]) if st == 0]
        assert len(ok) >= 4
        probs, lens = d["probs"][:, ok], [d["lens"][b] for b in ok]
        strings = [" ".join(i2c[k] for k in want[0][b]) for b in ok]
        bd0 = BeamDecoder(i2c, beam_width=W, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=d["alpha"])
        assert bd0._decoder.decode(torch.from_numpy(probs).transpose(0, 1), lens) == strings
        base = bd0.decode(torch.log(torch.from_numpy(probs)), lens)
        assert all(base) and len(base) == len(ok)
        for blank in (1, 31, 61):
            moved, _, old = synth.move_blank(probs, d["lm"], blank)
            bd = BeamDecoder({j: i2c[int(old[j])] for j in range(62)}, beam_width=W, blank_index=blank, space_idx=-1, lm_path=arpa, lm_alpha=d["alpha"])
            assert bd._decoder.decode(torch.from_numpy(moved).transpose(0, 1), lens) == strings, (name, blank)
            assert bd.decode(torch.log(torch.from_numpy(moved)), lens) == base, (name, blank)
            assert not np.isnan(bd._decoder.decode_ids(torch.from_numpy(moved).to(dev), lens, input_is_prob=True)[1]).any()
        if name == "mix62":
            zi = d["names"].index("zero_on_kept")
            zero = d["probs"][:, [zi]]
            for blank, dec in ((0, bd0), (61, bd)):
                z = synth.move_blank(zero, d["lm"], blank)[0] if blank else zero
                with pytest.raises(ValueError):
                    dec._decoder.decode(torch.from_numpy(z).transpose(0, 1), [d["lens"][zi]])
                with pytest.raises(ValueError):
                    dec.decode(torch.log(torch.from_numpy(z)), [d["lens"][zi]])          # log(0) = -inf, whose float32 exp is 0 again
