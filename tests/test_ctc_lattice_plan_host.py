"""ctcn_diag_ctc_lattice_plan / ops.ctc_lattice_plan: the launch behind the CTC lattice passes (ctc.hip: plan_ctc_lattice) held to a
restatement of its rule, and the two options of the wave-skewed lattice.  Pure arithmetic: no GPU."""
import ctypes

import pytest

from ctc_pytorch_amd import _lib, ops

LMAX = (0, 1, 31, 32, 63, 64, 95, 96, 127, 128, 2047)


@pytest.fixture
def options_put_back():
    before = {n: ops.get_option(n) for n in ("ctc_lattice_skew", "ctc_slow_wave")}
    yield
    for n, v in before.items():
        ops.set_option(n, v)


def _rule(Lmax, skew):
    S = 2 * Lmax + 1
    waves = -(-S // 64)
    if skew and S <= 256:
        return {"skewed": 1, "waves": waves, "ns": 1, "threads": 64 * waves}
    ns = -(-S // 256)
    return {"skewed": 0, "waves": waves, "ns": next(n for n in (1, 2, 4, 8, 16) if n >= ns), "threads": 256, "lds": 3 * S * 4}


@pytest.mark.parametrize("Lmax", LMAX)
def test_plan_follows_the_rule(options_put_back, Lmax):
    assert ops.get_option("ctc_lattice_skew") == 1                    # the default
    for skew in (1, 0):
        ops.set_option("ctc_lattice_skew", skew)
        p = ops.ctc_lattice_plan(Lmax)
        want = _rule(Lmax, skew)
        assert {k: p[k] for k in want} == want, (Lmax, skew, p)
        assert p["waves"] == -(-(2 * Lmax + 1) // 64)
        assert p["skewed"] == (1 if skew and Lmax <= 127 else 0)
        if p["skewed"]:
            assert p["waves"] <= 4 and 0 < p["lds"] <= 1024             # the ring and the two final states: a few hundred bytes
        else:
            assert p["lds"] == 3 * (2 * Lmax + 1) * 4                   # the classic path's three lattice rows, unchanged
        assert 2 <= p["skew"] <= 16                                     # frames a wave runs behind its predecessor: a constant of the build


def test_plan_rejects_bad_arguments():
    L = _lib.lib()
    out = (ctypes.c_int * 6)()
    o = ctypes.cast(out, ctypes.c_void_p)
    assert L.ctcn_diag_ctc_lattice_plan(10, o) == 0
    assert L.ctcn_diag_ctc_lattice_plan(-1, o) == -1
    assert L.ctcn_diag_ctc_lattice_plan(2048, o) == -1                   # S = 4097: past what any lattice kernel takes
    assert L.ctcn_diag_ctc_lattice_plan(10, None) == -1


def test_options_listed_and_clamped(options_put_back):
    names = ops.option_names()
    assert "ctc_lattice_skew" in names and "ctc_slow_wave" in names
    for given, kept in ((0, 0), (1, 1), (7, 1), (-3, 1)):
        ops.set_option("ctc_lattice_skew", given)
        assert ops.get_option("ctc_lattice_skew") == kept
    for given, kept in ((0, 0), (1, 1), (5, 5), (15, 15), (16, 15), (1 << 20, 15), (-1, 0)):
        ops.set_option("ctc_slow_wave", given)
        assert ops.get_option("ctc_slow_wave") == kept
