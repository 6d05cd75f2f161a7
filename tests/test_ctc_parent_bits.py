"""The CTC loss kernels after ctc.hip's refactor (one classic lattice walk behind a policy, one length contract, plan-then-launch): every
output bit of every entry point must be what the commit before it computed.

tests/golden/ctc_parent_bits.npz was written by tools/record_parent_bits.py from a build of that parent commit (its hash is in the file), never
from the code under test.  An output of up to FULL_MAX elements is held whole -- floats as their uint32 view, so that NaN rows compare -- a
larger one as the SHA-256 of its bytes.  Every output buffer is pre-filled with a sentinel and compared whole: a cell that one build writes and the
other does not is a difference.  Inputs come from seeded numpy RandomState generators on the host by arithmetic alone (no exp / log, whose last
bit may differ between machines); the fixture also holds a digest of every case's inputs, so that a change of the inputs is told apart from a
change of the kernels.

Cases (V = 8; B = 3 with ragged lengths on the skewed path, B = 2 on the long classic ones):
  skew_L<Lmax>   ctcn_ctc_fwd_ex without and with beta, then ctcn_ctc_grad_ex, for T in {1, 2, 5, 9, 13} (no chunk, a partial chunk, both sides
                 of the fast / slow chunk split): utterance 2 has exactly T frames and a label short enough for them, utterances 0 and 1 the full
                 and the half label (with repeats: the skip rule) on the fewest frames that hold them.  Lmax 1 .. 127: one wave, both sides
                 of a wave edge, four waves.
  classic_L<Lmax> option "ctc_lattice_skew" = 0: the same calls, plus ctcn_ctc_fwd, ctcn_ctc_bwd (in place), ctcn_ctc_fwd_both and ctcn_ctc_grad.
                 Lmax 3 .. 2047: NS = 1, 2, 2, 4, 8, 16 states per thread, on the fewest frames that hold the labels.
  edges_*        both paths, blank 0 and V - 1: an infeasible utterance, in_len = 0 with L = 0 and with L > 0, an input length outside the tensor
                 (NaN rows), under zero_infinity 0 / 1 and the reductions none / sum / mean.
  align_*        ctcn_ctc_align: the NS ladder (back-pointer rows in LDS for the short ones, in the workspace for the long ones), a long input
                 with a short label (workspace, several trace chunks), all-equal log-probs (ties everywhere), a -inf column, blank != 0."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import ctc_ref

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ctc_parent_bits.npz")
FULL_MAX = 4096          # elements: larger arrays are stored as a digest
SENTINEL = 12345.0
V = 8
SKEW_T = (1, 2, 5, 9, 13)
NONE, MEAN, SUM = 0, 1, 2

CASES = {}
for _L in (1, 31, 32, 63, 64, 127):
    CASES["skew_L%d" % _L] = ("skew", _L)
for _L in (3, 128, 200, 384, 900, 2047):
    CASES["classic_L%d" % _L] = ("classic", _L)
    CASES["align_L%d" % _L] = ("align", _L)
for _skew in (1, 0):
    for _blank in (0, V - 1):
        CASES["edges_skew%d_blank%d" % (_skew, _blank)] = ("edges", _skew, _blank)
CASES["align_longT"] = ("align_longT",)
CASES["align_ties"] = ("align_ties",)
CASES["align_ninf_column"] = ("align_ninf",)
CASES["align_blank7"] = ("align_blank",)
EXPECTED_NS = {3: 1, 128: 2, 200: 2, 384: 4, 900: 8, 2047: 16}


def _rs(name, salt=0):
    return np.random.RandomState(5000 + 16 * sorted(CASES).index(name) + salt)


def _lp(rs, T, B):
    """(T, B, V) float32 in (-6.05, -0.05]: un-normalised log-probs by arithmetic alone."""
    return (-(rs.random_sample((T, B, V)) * 6.0 + 0.05)).astype(np.float32)


def _batch(rs, labels, in_len, Lmax, blank, T=None):
    """labels: list of 1-D int64 arrays -> dict lp, tg (B, Lmax) padded with a valid class, il, tl, T, B, Lmax, blank."""
    B = len(labels)
    T = max(max(in_len), 1) if T is None else T
    tg = np.full((B, Lmax), (blank + 1) % V, dtype=np.int64)
    for i, l in enumerate(labels):
        tg[i, :len(l)] = l
    return dict(lp=_lp(rs, T, B), tg=tg, il=np.array(in_len, dtype=np.int64), tl=np.array([len(l) for l in labels], dtype=np.int64), T=T, B=B,
                Lmax=Lmax, blank=blank)


def _classes(blank):
    return [c for c in range(V) if c != blank]


def _skew_batch(name, Lmax, T):
    rs = _rs(name, SKEW_T.index(T))
    l0, l1 = ctc_ref.make_labels(rs, Lmax, _classes(0)), ctc_ref.make_labels(rs, Lmax // 2, _classes(0))
    l2 =ctc_ref.make_labels(rs, min(Lmax, T - 1), _classes(0), repeat=0.0)
    return _batch(rs, [l0, l1, l2], [max(T, ctc_ref.min_frames(l0)), max(T, ctc_ref.min_frames(l1)), T], Lmax, 0)


def _long_batch(name, Lmax, blank=0):
    rs = _rs(name)
    l0, l1 = ctc_ref.make_labels(rs, Lmax, _classes(blank)), ctc_ref.make_labels(rs, (Lmax + 1) // 2, _classes(blank))
    if ctc_ref.repeats(l0) == 0:
        l0[1] = l0[0]                                          # (the short ones: a repeated label by hand)
    return _batch(rs, [l0, l1], [ctc_ref.min_frames(l0), ctc_ref.min_frames(l1)], Lmax, blank)


EDGE_T, EDGE_LMAX = 9, 5


def _edge_batch(name, blank):
    """0: full, 1: infeasible (7 frames needed, 5 given), 2: no frames and no label, 3: no frames but a label, 4: in_len outside the tensor, 5: short."""
    rs = _rs(name)
    c = _classes(blank)
    labels = [np.array([c[0], c[1], c[2], c[1], c[0]]), np.array([c[0], c[0], c[1], c[1], c[2]]), np.array([], dtype=np.int64),
              np.array([c[3], c[4], c[5]]), np.array([c[0], c[1]]), np.array([c[6], c[6]])]
    return _batch(rs, [np.asarray(l, dtype=np.int64) for l in labels], [9, 5, 0, 0, EDGE_T + 1, 4], EDGE_LMAX, blank, T=EDGE_T)


def inputs(name):
    """-> list of (tag, batch) of a case"""
    kind = CASES[name][0]
    if kind == "skew":
        return [("T%d" % T, _skew_batch(name, CASES[name][1], T)) for T in SKEW_T]
    if kind in ("classic", "align"):
        return [("", _long_batch(name, CASES[name][1]))]
    if kind == "edges":
        return [("", _edge_batch(name, CASES[name][2]))]
    rs = _rs(name)
    if kind == "align_longT":                                  # rows in the workspace: S = 7, one word per frame, more than 15 337 frames
        b = _batch(rs, [np.array([1, 2, 2]), np.array([3])], [15400, 9000], 3, 0)
    elif kind == "align_ties":
        b = _batch(rs, [np.array([1, 2, 2, 3]), np.array([4, 4])], [11, 6], 4, 0)
        b["lp"][:] = np.float32(-2.0)
    elif kind == "align_ninf":                                 # class 5: not in utterance 0's label, in utterance 1's (no alignment)
        b = _batch(rs, [np.array([1, 2, 2, 3]), np.array([4, 5])], [11, 6], 4, 0)
        b["lp"][:, :, 5] = -np.inf
    else:
        b = _long_batch(name, 40, blank=V - 1)
    b["tg"] = np.ascontiguousarray(b["tg"], dtype=np.int64)
    return [("", b)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs_digest(name):
    h = hashlib.sha256()
    for tag, b in inputs(name):
        for k in ("lp", "tg", "il", "tl"):
            h.update(np.ascontiguousarray(b[k]).tobytes())
    return h.hexdigest()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _lattice_calls(b, dev, legacy, grads):
    """The loss entry points on one batch -> {key: torch tensor on the device}.  grads: [(key, reduction, zero_infinity)] for ctcn_ctc_grad_ex."""
    from ctc_pytorch_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    T, B, Lmax, blank = b["T"], b["B"], b["Lmax"], b["blank"]
    lp, tg, il, tl = (torch.from_numpy(b[k]).to(dev) for k in ("lp", "tg", "il", "tl"))
    S = 2 * Lmax + 1
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev)
    out = {}
    a, n = full(T, B, S), full(B)
    _lib.check(L.ctcn_ctc_fwd_ex(_P(lp), _P(tg), _P(il), _P(tl), _P(a), None, _P(n), T, B, V, Lmax, blank, st), "ctc_fwd_ex")
    out.update({"a/alpha": a, "a/nll": n})
    a, bt, n = full(T, B, S), full(T, B, S), full(B)
    _lib.check(L.ctcn_ctc_fwd_ex(_P(lp), _P(tg), _P(il), _P(tl), _P(a), _P(bt), _P(n), T, B, V, Lmax, blank, st), "ctc_fwd_ex")
    out.update({"ab/alpha": a, "ab/beta": bt, "ab/nll": n})
    scalar = torch.full((1,), 0.375, device=dev)
    vector = torch.from_numpy((0.25 + 0.125 * np.arange(B)).astype(np.float32)).to(dev)
    for key, reduction, zinf in grads:
        g = full(T, B, V)
        gs = vector if reduction == NONE else scalar
        _lib.check(L.ctcn_ctc_grad_ex(_P(lp), _P(tg), _P(il), _P(tl), _P(a), _P(bt), _P(n), _P(gs), int(reduction == NONE), reduction, zinf, blank,
                                      _P(g), T, B, V, Lmax, st), "ctc_grad_ex")
        out[key] = g
    if legacy:
        assert blank == 0
        a, n, g = full(T, B, S), full(B), full(T, B, V)
        _lib.check(L.ctcn_ctc_fwd(_P(lp), _P(tg), _P(il), _P(tl), _P(a), _P(n), T, B, V, Lmax, st), "ctc_fwd")
        out.update({"fwd/alpha": a.clone(), "fwd/nll": n})
        _lib.check(L.ctcn_ctc_bwd(_P(lp), _P(tg), _P(il), _P(tl), _P(a), _P(n), _P(scalar), _P(g), T, B, V, Lmax, st), "ctc_bwd")
        out.update({"bwd/alpha_beta": a, "bwd/grad": g})
        a, bt, n, g = full(T, B, S), full(T, B, S), full(B), full(T, B, V)
        _lib.check(L.ctcn_ctc_fwd_both(_P(lp), _P(tg), _P(il), _P(tl), _P(a), _P(bt), _P(n), T, B, V, Lmax, st), "ctc_fwd_both")
        _lib.check(L.ctcn_ctc_grad(_P(lp), _P(tg), _P(il), _P(tl), _P(a), _P(bt), _P(n), _P(scalar), _P(g), T, B, V, Lmax, st), "ctc_grad")
        out.update({"both/alpha": a, "both/beta": bt, "both/nll": n, "both/grad": g})
    return out


def _align_call(b, dev):
    from ctc_pytorch_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    T, B, Lmax, blank = b["T"], b["B"], b["Lmax"], b["blank"]
    lp, tg, il, tl = (torch.from_numpy(b[k]).to(dev) for k in ("lp", "tg", "il", "tl"))
    paths, fs = torch.full((B, T), -7, dtype=torch.int32, device=dev), torch.full((B, T), SENTINEL, device=dev)
    sc, ok = torch.full((B,), SENTINEL, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    starts, ends = torch.full((B, Lmax), -7, dtype=torch.int32, device=dev), torch.full((B, Lmax), -7, dtype=torch.int32, device=dev)
    need = L.ctcn_ctc_align_ws_bytes(T, B, Lmax)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    _lib.check(L.ctcn_ctc_align(_P(lp), _P(tg), _P(il), _P(tl), _P(paths), _P(fs), _P(sc), _P(ok), _P(starts), _P(ends), T, B, V, Lmax, blank,
                                _P(ws), need, st), "ctc_align")
    return {"paths": paths, "frame_scores": fs, "score": sc, "ok": ok, "starts": starts, "ends": ends, "ws_bytes": torch.tensor([need])}


EDGE_GRADS = [("grad/%s_zinf%d" % (n, z), r, z) for z in (0, 1) for n, r in (("none", NONE), ("sum", SUM), ("mean", MEAN))]


def run_case(name, dev):
    """-> {key: numpy array}; floats as their uint32 view"""
    from ctc_pytorch_amd import ops
    kind = CASES[name][0]
    skew = {"skew": 1, "classic": 0, "edges": CASES[name][1] if kind == "edges" else 1}.get(kind, ops.get_option("ctc_lattice_skew"))
    old = ops.get_option("ctc_lattice_skew")
    out = {}
    try:
        ops.set_option("ctc_lattice_skew", skew)
        for tag, b in inputs(name):
            if kind.startswith("align"):
                res = _align_call(b, dev)
            else:
                if kind != "edges":
                    assert ops.ctc_lattice_plan(b["Lmax"])["skewed"] == skew, name
                res = _lattice_calls(b, dev, legacy=kind == "classic", grads=EDGE_GRADS if kind == "edges" else [("ab/grad", SUM, 0)])
            torch.cuda.synchronize()
            for k, t in res.items():
                a = t.cpu().numpy()
                out[(tag + "/" if tag else "") + k] = a.view(np.uint32) if a.dtype == np.float32 else a
    finally:
        ops.set_option("ctc_lattice_skew", old)
    return out


@pytest.fixture(scope="module")
def parent():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def check_claims(name):
    """The cases are what they claim to be (host arithmetic and tests/ctc_ref.py only); the recorder runs this before it writes anything."""
    kind = CASES[name][0]
    for tag, b in inputs(name):
        assert b["lp"].dtype == np.float32 and b["tg"].dtype == np.int64 and b["tg"].shape == (b["B"], b["Lmax"])
        feasible = [int(b["il"][i]) >= ctc_ref.min_frames(b["tg"][i, :b["tl"][i]]) for i in range(b["B"])]
        if kind == "skew":
            assert b["B"] == 3 and all(feasible) and int(b["il"][2]) == int(tag[1:]) and len(set(b["tl"].tolist())) > 1, (name, tag)
            assert 2 * b["Lmax"] + 1 <= 256
            if b["Lmax"] > 3:
                assert ctc_ref.repeats(b["tg"][0]) > 0, "no repeated label: the skip rule is not exercised"
        elif kind in ("classic", "align"):
            assert b["B"] == 2 and all(feasible) and b["T"] == ctc_ref.min_frames(b["tg"][0]) and ctc_ref.repeats(b["tg"][0]) > 0
            assert min(16, 1 << max(0, int(np.ceil(np.log2((2 * b["Lmax"] + 1) / 256.0))))) == EXPECTED_NS[b["Lmax"]]
        elif kind == "edges":
            blank = b["blank"]
            assert feasible == [True, False, True, False, True, True] and not (b["tg"][:, :] == blank).any()
            assert b["il"].tolist() == [9, 5, 0, 0, b["T"] + 1, 4] and b["tl"].tolist() == [5, 5, 0, 3, 2, 2]
            for i, want_inf in ((0, False), (1, True), (5, False)):
                ref = ctc_ref.reference(b["lp"][:, i, :], b["tg"][i, :b["tl"][i]], int(b["il"][i]), blank)
                assert np.isinf(ref["nll"]) == want_inf, (name, i, ref["nll"])
        elif kind == "align_longT":
            assert b["T"] * 4 + (3 * 7 + 1026) * 4 > 64 * 1024 and b["T"] > 1024 and all(feasible)
        elif kind == "align_ties":
            assert len(np.unique(b["lp"])) == 1 and all(feasible)
        elif kind == "align_ninf":
            assert np.isinf(b["lp"][:, :, 5]).all() and 5 not in b["tg"][0, :b["tl"][0]] and 5 in b["tg"][1, :b["tl"][1]]
        elif kind == "align_blank":
            assert b["blank"] == V - 1 and not (b["tg"] == V - 1).any() and all(feasible)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_what_they_claim(name):
    check_claims(name)


def test_fixture_covers_every_case(parent):
    arrays, meta = parent
    assert len(meta["commit"]) >= 7 and sorted(meta["cases"]) == sorted(CASES)
    assert os.path.getsize(FIXTURE) <= max(os.path.getsize(os.path.join(os.path.dirname(FIXTURE), f)) for f in os.listdir(os.path.dirname(FIXTURE))
                                           if f != os.path.basename(FIXTURE))
    for name in CASES:
        assert meta["inputs"][name] == inputs_digest(name), "%s: the inputs are not the recorded ones (the generator changed, not the kernels)" % name
        for key in meta["cases"][name]:
            assert "%s/%s" % (name, key) in arrays or "%s/%s" % (name, key) in meta["digests"], (name, key)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_ctc_bits_are_the_parents(parent, dev, name):
    arrays, meta = parent
    got = run_case(name, dev)
    assert sorted(got) == sorted(meta["cases"][name]), (sorted(got), meta["cases"][name])
    bad = []
    for key, g in got.items():
        full = "%s/%s" % (name, key)
        if full in arrays:
            want = arrays[full]
            assert want.dtype == g.dtype and want.shape == g.shape, (key, want.dtype, g.dtype, want.shape, g.shape)
            if not np.array_equal(want, g):
                bad.append("%s: %d of %d elements differ" % (key, int((want != g).sum()), g.size))
        elif digest(g) != meta["digests"][full]:
            bad.append("%s: the digest of its %d elements differs" % (key, g.size))
    assert not bad, "; ".join(bad)
