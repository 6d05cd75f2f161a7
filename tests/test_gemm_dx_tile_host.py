"""ctcn_diag_dx_plan: the decision behind ctcn_gemm_dx (gemm.hip: plan_dx) -- whether the dx product of a recurrent layer takes the 256 x 320
float32-A tile or goes to ctcn_gemm(0, 0, ...) as before.  Pure arithmetic: no GPU.

Where the expected values come from: not from the function.  The tile is taken when ceil(tiles_wide / CUs) * r < ceil(tiles_128 / CUs) with
tiles_wide = ceil(M / 256) * N / 320, tiles_128 = ceil(M / 256) * ceil(N / 128) and r the cost of a wide tile in 256 x 128 tiles; every row
below holds for ANY 1 < r < 2 (a wide tile does 2.5 times the work of a narrow one in less than twice its time, and more than its time), on
256 CUs:
    M = 25 600, N = 640: 200 wide tiles = 1 round, 500 narrow = 2 rounds: r < 2            -> wide
    M = 51 200:          400 = 2 rounds, 1 000 = 4 rounds: 2 r < 4                          -> wide
    M = 13 312:          104 = 1 round, 260 = 2 rounds                                      -> wide   (the ragged loop's smallest M)
    M = 12 800:          100 = 1 round, 250 = 1 round: r < 1 is false                       -> not
    M = 6 400:           50 and 125: one round each                                         -> not
"""
import ctypes

import pytest

WS = 1 << 30
B_PLANES = 2 * 640 * 2560 * 2          # hi + lo bf16 planes of a 640 x 2 560 B: what the workspace must hold


def dx_plan(M, N=640, K=2560, lda=None, prec=1, amod=0, ws=WS, cus=256):
    from ctc_pytorch_amd import _lib
    out = (ctypes.c_int * 4)()
    rc = _lib.lib().ctcn_diag_dx_plan(M, N, K, K if lda is None else lda, prec, amod, 0 if ws is None else 1, ws or 0, cus,
                                      ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, (rc, _lib.lib().ctcn_last_error())
    return dict(zip(("eligible", "wide", "tiles_wide", "tiles_128"), out))


@pytest.fixture
def options():
    """set(name, value) for the test; every option it moved is put back."""
    from ctc_pytorch_amd import ops
    old = {}

    def set_(name, value):
        old.setdefault(name, ops.get_option(name))
        ops.set_option(name, value)
    yield set_
    for name, value in old.items():
        ops.set_option(name, value)


def test_default_option_and_tile_counts():
    from ctc_pytorch_amd import ops
    assert ops.get_option("gemm_dx_wide") == 1 and "gemm_dx_wide" in ops.option_names()
    p = dx_plan(25600)
    assert p == dict(eligible=1, wide=1, tiles_wide=200, tiles_128=500)
    assert dx_plan(300, N=960, K=160)["tiles_wide"] == 6 and dx_plan(300, N=960, K=160)["tiles_128"] == 16


@pytest.mark.parametrize("M,wide", [(25600, 1), (51200, 1), (13312, 1), (12800, 0), (6400, 0)])
def test_rounds_rule(M, wide):
    p = dx_plan(M)
    assert p["eligible"] == 1 and p["wide"] == wide, p


@pytest.mark.parametrize("what,kw", [("N = 768 is no multiple of 320", dict(N=768)), ("N = 636", dict(N=636)), ("precision 0", dict(prec=0)),
                                     ("K < 64", dict(K=32)), ("K % 4", dict(K=2562, lda=2564)), ("lda % 4", dict(lda=2561)),
                                     ("A not 16-byte aligned", dict(amod=4)), ("no workspace", dict(ws=None)),
                                     ("workspace smaller than B's planes", dict(ws=B_PLANES - 1))])
def test_ineligible_calls_never_take_the_tile(what, kw, options):
    for opt in (1, 2):
        options("gemm_dx_wide", opt)
        p = dx_plan(25600, **kw)
        assert p["eligible"] == 0 and p["wide"] == 0, (what, opt, p)
    # the same call without the condition is eligible: the row above tests that condition
    assert dx_plan(25600)["eligible"] == 1
    assert dx_plan(25600, ws=B_PLANES)["wide"] == 1


def test_bf16_single_mode_keeps_the_narrow_tile(options):
    options("gemm_bf16_single", 1)
    options("gemm_dx_wide", 2)
    p = dx_plan(25600)
    assert p["eligible"] == 0 and p["wide"] == 0, p


def test_option_values(options):
    options("gemm_dx_wide", 0)
    assert [dx_plan(M)["wide"] for M in (25600, 51200, 300)] == [0, 0, 0] and dx_plan(25600)["eligible"] == 1
    options("gemm_dx_wide", 2)
    p = dx_plan(300)
    assert p["eligible"] == 1 and p["wide"] == 1 and p["tiles_wide"] == 4, p
    assert dx_plan(12800)["wide"] == 1
    assert dx_plan(300, N=768)["wide"] == 0            # ... wherever ELIGIBLE
    options("gemm_dx_wide", 7)                         # the setter clamps
    from ctc_pytorch_amd import ops
    assert ops.get_option("gemm_dx_wide") == 2


def test_bad_arguments():
    from ctc_pytorch_amd import _lib
    out = (ctypes.c_int * 4)()
    o = ctypes.cast(out, ctypes.c_void_p)
    L = _lib.lib()
    assert L.ctcn_diag_dx_plan(0, 640, 2560, 2560, 1, 0, 1, WS, 256, o) != 0
    assert L.ctcn_diag_dx_plan(256, 640, 2560, 2560, 1, 0, 1, WS, 0, o) != 0
    assert L.ctcn_diag_dx_plan(256, 640, 2560, 2560, 1, 16, 1, WS, 256, o) != 0
    assert L.ctcn_diag_dx_plan(256, 640, 2560, 2560, 1, 0, 1, WS, 256, None) != 0
