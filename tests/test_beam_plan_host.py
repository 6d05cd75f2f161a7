"""ctcn_diag_beam_plan / ops.beam_plan: the decisions behind ctcn_beam_decode (decode.hip: plan_beam) -- fast kernel, its occ2 build or the
generic kernel; the instantiation; the dynamic LDS each kernel is launched with; the workspace.  Pure arithmetic: no GPU.

The rules are restated here, once, from the kernels' contracts and not from the function:
  * fast kernel: 832 candidate threads with at most 4 candidates each; beam width <= 60; V <= 256; LDS = alpha * LM (V+1)^2 doubles | cand
    W V doubles | ln p 2 V doubles | mslot W V ints | frame list T ints | trie slots uints, within 144 KB (68 KB for the occ2 builds, two
    workgroups per CU); the trie takes the largest power of two <= 16 384 that fits next to an LM table of at most 40 KB, the table goes to
    LDS if it then still fits, and beam_occ2 = 2 leaves it in global memory;
  * generic kernel: one thread per beam slot in 256 / 512 / 1 024 threads; dynamic LDS = ln p V doubles + 10 doubles and 10 ints per beam
    slot (W rounded up to 64) + a double and an int per survivor (max(1 024, 2 slots)); then the candidate table, then the LM table
    (+ 8 bytes), each if it fits the device's LDS per workgroup with 256 bytes to spare.
The static LDS of the three generic instantiations (sample inputs of the arithmetic: the decode call asks the runtime for the current
kernels' sizes, which may differ by a few bytes) and the workspace sizes of tests/golden/beam_ws_bytes.json were recorded from the build
before plan_beam existed."""
import json
import os

import pytest

G = os.path.join(os.path.dirname(__file__), "golden")
GENERIC_STATIC_LDS = {256: 176, 512: 448, 1024: 1376}
BEAM_OPTIONS = {"beam_fast": 1, "beam_occ2": 0, "beam_generic_threads": 0, "beam_cand_global": 0}


@pytest.fixture
def options():
    """set(name, value) for the test; every beam option goes back to its default."""
    from ctc_pytorch_amd import ops
    yield ops.set_option
    for k, v in BEAM_OPTIONS.items():
        ops.set_option(k, v)


def fast_rule(T, V, W, occ2):
    """(ok, lm_lds, trie_slots, npt, LDS bytes) of the fast kernel; ok false = ctcn_beam_decode takes the generic kernel instead."""
    npt = -(-W * V // 832)
    core = (W * V + 2 * V) * 8 + (W * V + T) * 4
    lm = (V + 1) * (V + 1) * 8
    budget = (68 if occ2 else 144) * 1024
    want_lm = lm <= 40 * 1024 and occ2 != 2
    slots = 16384
    while slots > 1024 and core + slots * 4 + (lm if want_lm else 0) > budget:
        slots >>= 1
    lm_lds = occ2 != 2 and core + slots * 4 + lm <= budget
    lds = core + slots * 4 + (lm if lm_lds else 0)
    ok = W <= 60 and 0 < npt <= 4 and V <= 256 and W * T + 2 < (1 << 24) and T < (1 << 22) and lds <= budget
    return ok, lm_lds, slots, npt if npt <= 4 else 0, lds


def generic_rule(V, W, forced, cand_global, lds_max):
    need = (1024 if W > 64 or W * V > 3500 else 256) if forced == 0 else max(forced, W)
    threads = 1024 if need > 512 else 512 if need > 256 else 256
    static = GENERIC_STATIC_LDS[threads]
    wcap = (W + 63) // 64 * 64
    smax = max(1024, 2 * wcap)
    base = V * 8 + wcap * (10 * 8 + 10 * 4) + smax * (8 + 4)
    cand, lm = W * V * 8, (V + 1) * (V + 1) * 8 + 8
    cand_in_lds = static + base + 256 + cand <= lds_max and not cand_global
    lm_in_lds = static + base + 256 + (cand if cand_in_lds else 0) + lm <= lds_max
    lds = base + (cand if cand_in_lds else 0) + (lm if lm_in_lds else 0)
    return dict(threads=threads, wcap=wcap, smax=smax, cand_in_lds=int(cand_in_lds), lm_in_lds=int(lm_in_lds), generic_lds=lds,
                generic_fits=int(static + lds <= lds_max))


@pytest.mark.parametrize("occ2", [0, 1, 2])
def test_fast_path_rule_on_a_grid(options, occ2):
    from ctc_pytorch_amd import ops
    options("beam_occ2", occ2)
    taken = 0
    for V in (3, 4, 5, 8, 16, 62, 70, 71, 256, 257):
        for W in (1, 2, 20, 52, 60, 61):
            for T in (1, 70, 800, 4000):
                ok, lm_lds, slots, npt, lds = fast_rule(T, V, W, occ2)
                p = ops.beam_plan(T, 2, V, W, generic_static_lds=GENERIC_STATIC_LDS[1024])
                got = (p["ok"], p["lm_lds"], p["trie_slots"], p["npt"], p["lds"])
                assert got == (int(ok), int(lm_lds), slots, npt, lds), (V, W, T, occ2, got)
                assert p["path"] == ((1 if occ2 else 0) if ok else 2) and p["rc"] == 0, (V, W, T, occ2)
                taken += ok
    assert 0 < taken < 10 * 6 * 4


# tests/test_gpu_kernels.py OCC2_CASES: (V, T, W, {occ2: (lm_lds, trie_slots)} or None); every one is meant for the fast kernel
OCC2_CASES = [(62, 800, 20, {1: (True, 4096), 2: (False, 8192)}), (62, 160, 52, {1: (False, 1024), 2: (False, 4096)}), (3, 70, 2, None),
              (4, 70, 5, None), (8, 70, 33, None), (5, 70, 52, None), (62, 160, 20, None)]


@pytest.mark.parametrize("V,T,W,expect", OCC2_CASES)
def test_occ2_cases_take_the_fast_kernel_they_were_written_for(options, V, T, W, expect):
    from ctc_pytorch_amd import ops
    for occ2 in (0, 1, 2):
        options("beam_occ2", occ2)
        p = ops.beam_plan(T, 8, V, W)
        assert p["ok"] == 1 and p["path"] == (1 if occ2 else 0), (V, T, W, occ2)
        assert (p["lm_lds"], p["trie_slots"]) == tuple(int(v) for v in fast_rule(T, V, W, occ2)[1:3])
        if expect is not None and occ2:
            assert (bool(p["lm_lds"]), p["trie_slots"]) == expect[occ2], (V, T, W, occ2)
    options("beam_fast", 0)
    assert ops.beam_plan(T, 8, V, W, generic_static_lds=GENERIC_STATIC_LDS[256])["path"] == 2


@pytest.mark.parametrize("lds_max", [65536, 163840])
def test_generic_plan(options, lds_max):
    from ctc_pytorch_amd import ops
    options("beam_fast", 0)
    unsupported = 0
    for forced in (0, 256, 512, 1024):
        for cand_global in (0, 1):
            options("beam_generic_threads", forced)
            options("beam_cand_global", cand_global)
            for V in (6, 62, 257):
                for W in (1, 20, 61, 130, 200, 256, 257, 300, 512, 513, 1024):
                    want = generic_rule(V, W, forced, cand_global, lds_max)
                    p = ops.beam_plan(70, 3, V, W, lds_max, GENERIC_STATIC_LDS[want["threads"]])
                    assert p["path"] == 2 and {k: p[k] for k in want} == want, (V, W, forced, cand_global, p)
                    assert want["threads"] >= W or want["threads"] == 1024
                    assert p["rc"] == (0 if GENERIC_STATIC_LDS[want["threads"]] + p["generic_lds"] <= lds_max else -3)
                    unsupported += p["rc"] != 0
    assert (unsupported > 0) == (lds_max == 65536)             # (W = 1 024 needs 146 KB for its beam state alone)
    options("beam_generic_threads", 256)
    assert ops.beam_plan(70, 3, 62, 300, lds_max, GENERIC_STATIC_LDS[512])["threads"] >= 512      # (one thread per beam slot)


def test_default_threads_and_placement_at_the_reference_width(options):
    """W = 200, V = 62 on the MI355X's 160 KB: 1 024 threads; 42 KB of beam state and the 97-KB candidate table are in LDS, which leaves no
    room for the 31-KB LM table (W = 61: both fit); with 64 KB of LDS neither table fits."""
    from ctc_pytorch_amd import ops
    options("beam_fast", 0)
    p = ops.beam_plan(800, 128, 62, 200, 163840, GENERIC_STATIC_LDS[1024])
    assert (p["threads"], p["cand_in_lds"], p["lm_in_lds"], p["rc"]) == (1024, 1, 0, 0)
    p = ops.beam_plan(800, 128, 62, 61, 163840, GENERIC_STATIC_LDS[1024])      # (3 782 candidates per frame: 1 024 threads as well)
    assert (p["threads"], p["cand_in_lds"], p["lm_in_lds"], p["rc"]) == (1024, 1, 1, 0)
    p = ops.beam_plan(800, 128, 62, 200, 65536, GENERIC_STATIC_LDS[1024])
    assert (p["threads"], p["cand_in_lds"], p["lm_in_lds"], p["rc"]) == (1024, 0, 0, 0)


def test_workspace_is_the_larger_of_the_two_plans_and_unchanged(options):
    from ctc_pytorch_amd import _lib, ops
    with open(os.path.join(G, "beam_ws_bytes.json")) as f:
        rows = json.load(f)["rows"]
    assert len(rows) == 720
    L = _lib.lib()
    for fast in (1, 0):                                     # (what a call must provide does not depend on the options at decode time)
        options("beam_fast", fast)
        for T, B, V, W, want in rows:
            p = ops.beam_plan(T, B, V, W)
            assert L.ctcn_beam_ws_bytes(T, B, V, W) == max(p["ws_fast"], p["ws_generic"]) == want, (T, B, V, W)


def test_bad_arguments_are_refused():
    import ctypes
    from ctc_pytorch_amd import _lib
    out = (ctypes.c_int * 19)()
    o = ctypes.cast(out, ctypes.c_void_p)
    L = _lib.lib()
    assert L.ctcn_diag_beam_plan(70, 2, 62, 20, 163840, 176, o) == 0
    for bad in ((0, 2, 62, 20, 163840, 176), (70, 0, 62, 20, 163840, 176), (70, 2, 1, 20, 163840, 176), (70, 2, 62, 0, 163840, 176),
                (70, 2, 62, 1025, 163840, 176), (70, 2, 62, 20, 0, 176), (70, 2, 62, 20, 163840, -1)):
        assert L.ctcn_diag_beam_plan(*bad, o) == -1, bad
    assert L.ctcn_diag_beam_plan(70, 2, 62, 20, 163840, 176, None) == -1
