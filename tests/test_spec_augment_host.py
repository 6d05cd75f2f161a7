"""SpecAugment without a GPU: ctcn_spec_augment_plan and ctcn_spec_augment_host (the interval and interpolation code the kernel is compiled
from) against the numpy restatement of the contract (tests/spec_augment_ref.py), the limits of every entry point, the generator
mapping's coverage, and the driver plumbing.  The demand is bit-identity: the draws are integer arithmetic and every float64 operation
of the warp is rounded on its own."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_augment_ref as SR  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

FULL = dict(warp_window=6, num_freq_masks=2, freq_width=7, num_time_masks=2, time_width=10, time_ratio=0.5, fill=-1.5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


PLAN_CASES = [
    # (T, F, seed, utt_index, options)
    (0, 5, 1, 0, FULL), (1, 5, 1, 1, FULL),
    (12, 5, 3, 2, FULL),                                               # T = 2 W: no warp
    (13, 5, 3, 2, FULL),                                               # T = 2 W + 1: c is W
    (70, 1, 9, 4, FULL),                                               # F = 1
    (70, 5, 9, 5, dict(FULL, freq_width=100)),                         # freq_width > F
    (70, 81, 9, 6, dict(FULL, time_ratio=0.01)),                       # floor(0.01 * 70) = 0: cap = 0
    (300, 81, 11, 7, dict(FULL, num_freq_masks=8, num_time_masks=32)),
    (300, 81, 11, (1 << 32) + 12345, SR.DEFAULTS),                     # an utterance index beyond 2^32
    (300, 81, 11, (1 << 56) + 3, SR.DEFAULTS),                         # (u << 8 wraps: still the same 64-bit arithmetic)
    (300, 81, 0xFEDCBA9876543210, 8, SR.DEFAULTS),                     # a seed with high bits set
    (800, 81, 2 ** 63 + 5, 9, dict(SR.DEFAULTS, time_ratio=1.0, time_width=1000)),
    (23, 81, 5, 1, FULL), (70, 81, 5, 0, FULL),
]


@pytest.mark.parametrize("case", range(len(PLAN_CASES)))
def test_plan_is_the_restatement(case):
    T, F, seed, u, kw = PLAN_CASES[case]
    got, want = ops.spec_augment_plan(T, F, seed, u, **kw), SR.plan(T, F, seed, u, **kw)
    assert got == want
    assert features.SpecAugment(seed=seed, **kw).plan(T, F, u) == want


def test_plan_edges():
    """What the edge cases of the grid above must give, whatever the words drawn."""
    assert ops.spec_augment_plan(12, 5, 3, 2, **FULL)["warp"] is None
    empty = ops.spec_augment_plan(0, 5, 1, 0, **FULL)
    assert empty["warp"] is None and empty["time"] == [(0, 0), (0, 0)]
    for u in range(20):
        c, w = ops.spec_augment_plan(13, 5, 3, u, **FULL)["warp"]
        assert c == 6 and 1 <= w <= 11
        assert all(n == 0 for _, n in ops.spec_augment_plan(70, 81, 9, u, **dict(FULL, time_ratio=0.01))["time"])
        assert all(n in (0, 1) and 0 <= f0 <= 1 - n for f0, n in ops.spec_augment_plan(70, 1, 9, u, **FULL)["freq"])


def _utt(T, F, seed):
    """Random float32 frames with neighbouring frames of very different magnitude (the two products of an interpolation then differ by
    many binades: a fused multiply-add would show)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(T, F).astype(np.float32)
    x *= (10.0 ** rs.randint(-6, 7, size=(T, 1))).astype(np.float32)
    return x


@pytest.mark.parametrize("T,F,kw", [(70, 81, FULL), (23, 81, FULL), (37, 5, FULL), (11, 5, FULL), (1, 3, FULL), (0, 3, FULL),
                                    (64, 7, dict(warp_window=16)), (200, 13, dict(SR.DEFAULTS, fill=3.25))])
def test_host_twin_is_the_restatement_bit_for_bit(T, F, kw):
    x = _utt(T, F, 100 * T + F)
    lerped = copied = 0
    for seed, u in ((5, 0), (5, 1), (0xFEDCBA9876543210, (1 << 40) + 7)):
        got, want = ops.spec_augment_host(x, seed, u, **kw), SR.augment(x, seed, u, **kw)
        assert got.shape == want.shape == x.shape and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
        p = SR.plan(T, F, seed, u, **kw)
        if p["warp"]:
            c, w = p["warp"]
            rems = [(t * c) % w if t < w else ((t - w) * (T - c)) % (T - w) for t in range(T)]
            lerped += sum(r != 0 for r in rems)
            copied += sum(r == 0 for r in rems)
    if T > 2 * kw["warp_window"]:
        assert lerped > 0 and copied > 0                               # both branches of the warp were held to the restatement


def test_all_options_off_is_the_identity():
    x = _utt(41, 9, 2)
    assert np.array_equal(bits(ops.spec_augment_host(x, 7, 3)), bits(x))
    assert np.array_equal(bits(ops.spec_augment_host(x, 7, 3, freq_width=5, time_width=9, fill=2.0)), bits(x))      # widths without counts
    assert ops.spec_augment_plan(41, 9, 7, 3) == {"warp": None, "freq": [], "time": []}
    assert ops.spec_augment_host(np.zeros((0, 4), dtype=np.float32), 1, 2, **FULL).shape == (0, 4)


def test_limits_of_every_entry_point():
    L = _lib.lib()
    fake = ctypes.c_void_p(64)                                         # never dereferenced: every check comes before the launch
    ibuf = (ctypes.c_int32 * 80)()
    x = np.zeros((4, 3), dtype=np.float32)
    y = np.zeros((4, 3), dtype=np.float32)

    def rc(F=3, T=4, B=1, **kw):
        o = _lib.SpecAugOpts(**dict(dict(warp_window=0, num_freq_masks=0, freq_width=0, num_time_masks=0, time_width=0, time_ratio=1.0, fill=0.0), **kw))
        return (L.ctcn_spec_augment(fake, fake, ctypes.byref(o), 1, 0, fake, B, T, F, None),
                L.ctcn_spec_augment_plan(ctypes.byref(o), 1, 0, T, F, ibuf, ibuf, ibuf),
                L.ctcn_spec_augment_host(x.ctypes.data_as(ctypes.c_void_p), T, F, ctypes.byref(o), 1, 0, y.ctypes.data_as(ctypes.c_void_p)))

    for kw in (dict(warp_window=-1), dict(num_freq_masks=-1), dict(freq_width=-1), dict(num_time_masks=-1), dict(time_width=-1),
               dict(time_ratio=-0.25), dict(time_ratio=1.5), dict(time_ratio=float("nan")), dict(fill=float("inf")), dict(fill=float("-inf")),
               dict(fill=float("nan")), dict(F=0), dict(F=-2), dict(T=(1 << 30) + 1), dict(T=-1)):
        assert rc(**kw) == (-1, -1, -1), kw
    for kw in (dict(num_freq_masks=9), dict(num_time_masks=33), dict(F=65537)):
        assert rc(**kw) == (-3, -3, -3), kw
    assert rc(B=0)[0] == -1 and rc(B=65536)[0] == -1 and rc(B=-1)[0] == -1
    o = _lib.SpecAugOpts(time_ratio=1.0)
    assert L.ctcn_spec_augment(fake, fake, None, 1, 0, fake, 1, 4, 3, None) == -1
    assert L.ctcn_spec_augment(None, fake, ctypes.byref(o), 1, 0, fake, 1, 4, 3, None) == -1
    assert L.ctcn_spec_augment(fake, None, ctypes.byref(o), 1, 0, fake, 1, 4, 3, None) == -1
    assert L.ctcn_spec_augment(fake, fake, ctypes.byref(o), 1, 0, None, 1, 4, 3, None) == -1
    assert L.ctcn_spec_augment(fake, fake, ctypes.byref(o), 1, 0, fake, 1, 4, 3, None) == -1           # out aliases feats
    assert L.ctcn_spec_augment_plan(None, 1, 0, 4, 3, ibuf, ibuf, ibuf) == -1
    assert L.ctcn_spec_augment_plan(ctypes.byref(o), 1, 0, 4, 3, None, None, None) == -1
    assert L.ctcn_spec_augment_host(None, 4, 3, ctypes.byref(o), 1, 0, y.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.ctcn_spec_augment_host(x.ctypes.data_as(ctypes.c_void_p), 4, 3, None, 1, 0, y.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.ctcn_spec_augment_host(x.ctypes.data_as(ctypes.c_void_p), 4, 3, ctypes.byref(o), 1, 0, None) == -1
    assert L.ctcn_spec_augment_host(x.ctypes.data_as(ctypes.c_void_p), 4, 3, ctypes.byref(o), 1, 0, x.ctypes.data_as(ctypes.c_void_p)) == -1
    # the limits themselves are accepted: 8 frequency masks, 32 time masks
    assert L.ctcn_spec_augment_plan(ctypes.byref(_lib.SpecAugOpts(num_freq_masks=8, num_time_masks=32, time_ratio=1.0)), 1, 0, 4, 3, ibuf, ibuf, ibuf) == 0
    # the public functions: the library's codes as RuntimeError, an unknown option as TypeError, a CPU tensor refused
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.spec_augment_plan(10, 3, 1, 0, num_freq_masks=9)
    with pytest.raises(RuntimeError, match="rc=-1"):
        ops.spec_augment_host(x, 1, 0, time_ratio=2.0)
    with pytest.raises(TypeError, match="unknown option"):
        ops.spec_augment_plan(10, 3, 1, 0, freq_masks=2)
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spec_augment(torch.zeros(1, 4, 3), [4], 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        features.SpecAugment(**SR.DEFAULTS)(torch.zeros(1, 4, 3), [4])


COVERAGE_SEED = 2019


def test_generator_mapping_covers_every_length_and_shift():
    """A condition on rnd(), not a measurement: over 2000 utterance indices under one seed every frequency-mask length 0 .. freq_width and
    every warp shift -(W - 1) .. W - 1 occurs, and no interval leaves [0, F) or [0, T).  The restatement alone meets it under this seed
    (asserted first); the library's plans are then the restatement's."""
    T, F, kw = 300, 81, SR.DEFAULTS
    W, fw = kw["warp_window"], kw["freq_width"]
    want = [SR.plan(T, F, COVERAGE_SEED, u, **kw) for u in range(2000)]
    assert {n for p in want for _, n in p["freq"]} == set(range(fw + 1))
    assert {p["warp"][1] - p["warp"][0] for p in want} == set(range(-(W - 1), W))
    cap = min(kw["time_width"], int(np.floor(np.float64(np.float32(kw["time_ratio"])) * T)))
    for p in want:
        c, w = p["warp"]
        assert W <= c < T - W and 1 <= w <= T - 1
        assert all(0 <= f0 and n >= 0 and f0 + n <= F for f0, n in p["freq"])
        assert all(0 <= t0 and 0 <= n <= cap and t0 + n <= T for t0, n in p["time"])
    assert [ops.spec_augment_plan(T, F, COVERAGE_SEED, u, **kw) for u in range(2000)] == want


def test_driver_plumbing():
    from ctc_pytorch_amd.steps import train_ctc

    class Off(object):
        seed = 4
    assert train_ctc.spec_augment(Off) is None

    class NoContext(Off):
        spec_augment = True
    with pytest.raises(ValueError, match="spec_augment.*device_context"):
        train_ctc.spec_augment(NoContext)

    class On(NoContext):
        device_context = True
    aug = train_ctc.spec_augment(On)
    assert isinstance(aug, features.SpecAugment) and aug.seed == 4 and aug.index == 0
    assert aug._kw() == dict(SR.DEFAULTS, fill=0.0) == dict(features.SpecAugment.DEFAULTS, fill=0.0)

    class Mapped(On):
        spec_augment = {"num_time_masks": 3, "time_width": 12, "fill": -2.0}
    aug = train_ctc.spec_augment(Mapped)
    assert aug._kw() == dict(warp_window=0, num_freq_masks=0, freq_width=0, num_time_masks=3, time_width=12, time_ratio=1.0, fill=-2.0)

    class Disabled(On):
        spec_augment = False
    assert train_ctc.spec_augment(Disabled) is None
    with pytest.raises(ValueError, match="unknown option"):
        features.SpecAugment.from_opts({"time_masks": 2})
    with pytest.raises(ValueError, match="expected true or a mapping"):
        features.SpecAugment.from_opts("yes")
    a = features.SpecAugment.from_opts(True, seed=9)
    assert a.seed == 9 and a.plan(300, 81, 5) == SR.plan(300, 81, 9, 5, **SR.DEFAULTS)
    assert features.SpecAugment(start_index=17).index == 17
