"""The device context stage's host side, without a GPU: the frame arithmetic and the float32 fractions against the loader's own, the delta
scales against the restatement of tests/frame_context_ref.py, the host twin ctcn_frame_context_host (the kernel's computation for one
utterance) bit for bit against the host loader path (no deltas) and against the float64 restatement (deltas), within the float32 worst case
of Kaldi's sequential form, the refusals, and the loader's base-feature mode."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_context_ref as FR  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import data_loader as DL  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

SKIPS, DOWNS = (0, 1, 2, 3, 5), (1, 2, 3, 4)
LENGTHS = (0, 1, 2, 3, 7, 20, 33)                   # shorter than every context and delta reach, equal to some, longer than all


vp, host_twin, same_bits = FR.vp, FR.host_twin, FR.same_bits


def test_frame_arithmetic_is_the_loaders():
    L = _lib.lib()
    for T in range(65):
        x = np.zeros((T, 1), dtype=np.float32)
        for skip in SKIPS:
            kept = DL.skip_feat(x, skip).shape[0]
            for nd in DOWNS:
                want = FR.host_path(x, 0, 0, skip, nd).shape[0]
                assert want == FR.context_frames(T, skip, nd) == -(-kept // nd) * nd
                assert L.ctcn_context_frames(T, skip, nd) == want == ops.context_frames(T, skip, nd), (T, skip, nd)
                assert features.FrameContext(0, 0, skip, nd).out_frames(T) == want
    for T in range(64):                                                # monotone: the padded length of a batch bounds every utterance's
        for skip in SKIPS:
            for nd in DOWNS:
                assert L.ctcn_context_frames(T, skip, nd) <= L.ctcn_context_frames(T + 1, skip, nd)
    assert L.ctcn_context_frames(-1, 1, 1) == -1 and L.ctcn_context_frames(4, -1, 1) == -1 and L.ctcn_context_frames(4, 1, 0) == -1
    assert L.ctcn_context_frames(2 ** 31 - 1, 1, 1000) == -3            # 2^31 - 1 rounded up to a multiple of 1000: beyond int
    with pytest.raises(ValueError):
        ops.context_frames(-1)


def test_fractions_are_create_inputs_float32_values():
    """create_input assigns the Python float t / tmax into a float32 element; the twin's (float)((double) n_out / (double) rows) is that."""
    for skip in SKIPS:
        for nd in DOWNS:
            tmax = FR.context_frames(64, skip, nd)
            items = [(torch.zeros((FR.context_frames(T, skip, nd), 1)), torch.zeros(1, dtype=torch.long), "u") for T in range(65)]
            _, sizes, _, _, _ = DL.create_input(items)
            sizes = sizes.numpy()
            for T in range(65):
                _, n, frac = host_twin(np.zeros((T, 1), dtype=np.float32), skip=skip, nd=nd, out_rows=tmax)
                assert np.float32(frac).view(np.uint32) == sizes[T].view(np.uint32), (T, skip, nd, frac, sizes[T])
    _, n, frac = host_twin(np.zeros((0, 3), dtype=np.float32), out_rows=0)
    assert n == 0 and frac == 0.0                                      # an empty batch has no fraction; the twin says 0


def test_delta_scales_are_the_restatement_bit_for_bit():
    L = _lib.lib()
    for window in range(1, 6):
        want = FR.delta_scales(2, window)
        for order in range(3):
            buf = np.full(2 * order * window + 3, -7.0, dtype=np.float32)
            assert L.ctcn_delta_scales(order, window, vp(buf)) == 2 * order * window + 1
            assert same_bits(buf[:-2], want[order]) and np.all(buf[-2:] == -7.0), (order, window, buf, want[order])
            assert same_bits(ops.delta_scales(order, window), want[order])
            if order:
                assert abs(float(want[order].astype(np.float64).sum())) <= 1e-7     # a delta filter has no DC gain
    assert L.ctcn_delta_scales(3, 2, vp(np.zeros(32, dtype=np.float32))) == -3
    assert L.ctcn_delta_scales(1, 6, vp(np.zeros(32, dtype=np.float32))) == -3
    assert L.ctcn_delta_scales(1, 0, vp(np.zeros(32, dtype=np.float32))) == -1
    assert L.ctcn_delta_scales(-1, 2, vp(np.zeros(32, dtype=np.float32))) == -1
    assert L.ctcn_delta_scales(1, 2, None) == -1


def test_known_delta_scales():
    assert same_bits(ops.delta_scales(0, 2), np.array([1.0], dtype=np.float32))
    assert same_bits(ops.delta_scales(1, 2), np.array([-0.2, -0.1, 0.0, 0.1, 0.2], dtype=np.float32))
    assert same_bits(ops.delta_scales(1, 1), np.array([-0.5, 0.0, 0.5], dtype=np.float32))
    # the order-2 filter is the order-1 filter applied twice: [4 4 1 -4 -10 -4 1 4 4] / 100
    assert np.allclose(ops.delta_scales(2, 2), np.array([4, 4, 1, -4, -10, -4, 1, 4, 4]) / 100.0, rtol=0, atol=1e-8)


@pytest.mark.parametrize("setting", FR.SETTINGS, ids=lambda s: "l%d_r%d_s%d_d%d" % s)
def test_copy_path_is_the_host_loader_bit_for_bit(setting):
    left, right, skip, nd = setting
    rs = np.random.RandomState(11)
    for F in (1, 13):
        for T in LENGTHS:
            x = rs.randn(T, F).astype(np.float32)
            want = FR.host_path(x, left, right, skip, nd)
            got, n, frac = host_twin(x, left, right, skip, nd)
            assert n == want.shape[0] and same_bits(got, want), (setting, F, T)
            assert frac == (1.0 if n else 0.0)
            # a longer buffer: the batch's other rows are zeros, the fraction is the collate's
            got, n, frac = host_twin(x, left, right, skip, nd, out_rows=n + 3)
            assert same_bits(got[:n], want) and np.all(got[n:] == 0.0) and np.float32(frac) == np.float32(n / (n + 3))


@pytest.mark.parametrize("order,window", [(1, 1), (1, 2), (2, 2), (2, 5)])
def test_delta_path_is_the_float64_restatement_and_within_kaldis_float32(order, window):
    rs = np.random.RandomState(order * 10 + window)
    worst = 0.0
    for F in (1, 13):
        for T in LENGTHS:
            x = (rs.randn(T, F) * 10.0 ** rs.uniform(-2, 2, size=(1, F))).astype(np.float32)
            want = FR.deltas64(x, order, window)
            got, n, _ = host_twin(x, order=order, window=window)
            assert n == T and same_bits(got, want), (order, window, F, T)
            k32, bound = FR.deltas_kaldi32(x, order, window)
            err = np.abs(got.astype(np.float64) - k32.astype(np.float64))
            assert np.all(err <= bound), (order, window, F, T, float((err - bound).max()))
            assert same_bits(got[:, :F], x) and same_bits(k32[:, :F], x)
            if T:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            # deltas, then splice, then skip and pad: the host loader path over the delta'd utterance
            full, n, _ = host_twin(x, 2, 1, 3, 4, order, window)
            assert same_bits(full, FR.host_path(want, 2, 1, 3, 4)), (order, window, F, T)
    print("deltas order %d window %d: largest |twin - Kaldi's float32 form| / bound = %.3g" % (order, window, worst))


def test_constant_and_ramp():
    """What a delta filter is for: a constant utterance has zero deltas (up to the rounding of the float32 scales, whose sum is within 1e-7
    of zero), a ramp of slope a has first delta a away from the edges."""
    x = np.full((12, 2), 3.25, dtype=np.float32)
    got, _, _ = host_twin(x, order=2, window=2)
    assert np.all(got[:, :2] == 3.25) and np.all(np.abs(got[:, 2:]) <= 3.25e-7)
    ramp = (0.5 * np.arange(12, dtype=np.float32))[:, None]
    got, _, _ = host_twin(ramp, order=2, window=2)
    assert np.allclose(got[2:-2, 1], 0.5, atol=1e-6) and np.allclose(got[4:-4, 2], 0.0, atol=1e-6)


def test_refusals():
    L = _lib.lib()
    x = np.zeros((4, 3), dtype=np.float32)
    out = np.zeros((64, 64 * 3 * 3), dtype=np.float32)

    def rc(F=3, T=4, rows=64, **kw):
        o = dict(left=0, right=0, skip=1, n_downsample=1, delta_order=0, delta_window=2)
        o.update(kw)
        opts = _lib.ContextOpts(**o)
        tile = L.ctcn_frame_context_tile(ctypes.byref(opts), F)
        host = L.ctcn_frame_context_host(vp(x), T, F, ctypes.byref(opts), vp(out), rows, None)
        # the launch refuses the same options before it looks at anything else (no device is touched)
        dev = L.ctcn_frame_context(None, None, ctypes.byref(opts), None, None, None, 1, 0, F, 0, None)
        return tile, host, dev

    for kw in (dict(left=-1), dict(right=-1), dict(skip=-1), dict(n_downsample=0), dict(delta_order=-1), dict(delta_window=0), dict(F=0)):
        assert rc(**kw) == (-1, -1, -1), kw
    for kw in (dict(left=65), dict(right=65), dict(skip=1025), dict(n_downsample=1025), dict(delta_order=3), dict(delta_window=6),
               dict(F=65537)):
        assert rc(**kw) == (-3, -3, -3), kw
    # a single output row whose span of frames does not fit the LDS; one frame of context less a side does, with a tile of one row
    assert L.ctcn_frame_context_tile(ctypes.byref(_lib.ContextOpts(left=15, right=15, skip=1, n_downsample=1, delta_order=2, delta_window=5)), 257) == -3
    assert L.ctcn_frame_context_tile(ctypes.byref(_lib.ContextOpts(left=14, right=14, skip=1, n_downsample=1, delta_order=2, delta_window=5)), 257) == 1
    assert L.ctcn_frame_context_tile(ctypes.byref(_lib.ContextOpts(left=0, right=2, skip=2, n_downsample=2, delta_order=0, delta_window=2)), 81) == 16
    assert L.ctcn_frame_context_tile(None, 3) == -1
    assert rc(T=-1)[1] == -1 and rc(rows=3)[1] == -1                    # a negative frame count; a buffer shorter than n_out
    # the launch's own arguments: NULL vectors, an empty batch, a Tout_max that is not the arithmetic's
    opts = _lib.ContextOpts(left=0, right=0, skip=2, n_downsample=1, delta_order=0, delta_window=2)
    assert L.ctcn_frame_context(None, None, ctypes.byref(opts), None, None, None, 1, 0, 3, 0, None) == -1
    fake = ctypes.c_void_p(64)                                          # never dereferenced: every check comes before the launch
    assert L.ctcn_frame_context(fake, fake, ctypes.byref(opts), fake, fake, fake, 0, 8, 3, 4, None) == -1
    assert L.ctcn_frame_context(fake, fake, ctypes.byref(opts), fake, fake, fake, 1, 8, 3, 5, None) == -1
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.frame_context_tile(3, delta_order=3)
    with pytest.raises(RuntimeError, match="rc=-3"):
        features.FrameContext(65, 0, 1, 1).out_dim(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_context(torch.zeros(1, 4, 3), [4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        features.FrameContext(0, 2, 2, 2)(torch.zeros(1, 4, 3), [4])
    assert features.FrameContext(0, 2, 2, 2).out_dim(81) == 243 and features.FrameContext(delta_order=2).out_dim(13) == 39


class _Opts(object):
    left_ctx, right_ctx, n_skip_frame, n_downsample = 0, 2, 2, 2


def _archive(tmp_path, lengths, F=5, seed=4):
    rs = np.random.RandomState(seed)
    mats = {"utt%d" % i: rs.randn(T, F).astype(np.float32) for i, T in enumerate(lengths)}
    ark, scp, lab, units = (str(tmp_path / n) for n in ("feats.ark", "feats.scp", "text", "units"))
    DL.write_kaldi_ark(ark, scp, mats)
    with open(units, "w") as f:
        f.write("a\nb\nc\n")
    with open(lab, "w") as f:
        for i, utt in enumerate(mats):
            f.write("%s %s\n" % (utt, " ".join("abc"[(i + k) % 3] for k in range(1 + i % 3))))
    return mats, DL.Vocab(units), scp, lab


def test_base_feature_loader_carries_the_integers(tmp_path):
    """The base-feature mode hands the archive's matrices and their exact frame counts on (no float32 fraction in between: that round trip is
    proven only up to 2000 frames); labels, label lengths and ids are the host loader's."""
    lengths = [9, 2500, 1, 7, 12, 3]
    mats, vocab, scp, lab = _archive(tmp_path, lengths)
    host = DL.SpeechDataLoader(DL.SpeechDataset(vocab, scp, lab, _Opts), batch_size=4, shuffle=False)
    base = DL.BaseFeatureLoader(DL.SpeechDataset(vocab, scp, lab, _Opts, base_features=True), batch_size=4, shuffle=False)
    assert len(host) == len(base) == 2
    keys = list(mats)
    for k, (h, b) in enumerate(zip(host, base)):
        data, frames, targets, target_sizes, utts = b
        assert frames.dtype == torch.int32 and frames.tolist() == lengths[4 * k:4 * k + 4]
        assert data.dtype == torch.float32 and tuple(data.shape) == (len(utts), max(frames.tolist()), 5)
        for i, utt in enumerate(utts):
            assert same_bits(data[i, :frames[i]].numpy(), mats[utt]) and np.all(data[i, frames[i]:].numpy() == 0.0)
        assert utts == h[4] == keys[4 * k:4 * k + 4] and torch.equal(targets, h[2]) and torch.equal(target_sizes, h[3])
        # what the device stage will make of it, by the host twin: the host loader's batch
        tmax = FR.context_frames(int(data.shape[1]), 2, 2)
        assert tmax == h[0].shape[1]
        for i in range(len(utts)):
            got, n, frac = host_twin(data[i, :frames[i]].numpy(), 0, 2, 2, 2, out_rows=tmax)
            assert same_bits(got, h[0][i].numpy()) and np.float32(frac).view(np.uint32) == h[1][i].numpy().view(np.uint32)
    with pytest.raises(ValueError, match="base_features"):
        DL.BaseFeatureLoader(DL.SpeechDataset(vocab, scp, lab, _Opts), batch_size=4)
    with pytest.raises(RuntimeError, match="GPU"):
        next(iter(DL.DeviceContext(base, "cpu", features.FrameContext(0, 2, 2, 2))))


def test_driver_keys():
    from ctc_pytorch_amd.steps import decode_ctc, make_feat, train_ctc
    assert train_ctc.device_context(_Opts) is None

    class On(_Opts):
        device_context = True
    ctx = train_ctc.device_context(On)
    assert (ctx.left, ctx.right, ctx.skip, ctx.n_downsample, ctx.delta_order) == (0, 2, 2, 2, 0)
    a = decode_ctc.arg_parser().parse_args(["--conf", "x", "--device-context"])
    assert decode_ctc.apply_argv({}, a) == {"device_context": True}
    assert "device_context" not in decode_ctc.apply_argv({}, decode_ctc.arg_parser().parse_args(["--conf", "x"]))
    for bad in (["--delta-order", "3"], ["--delta-order", "-1"], ["--delta-order", "1", "--delta-window", "0"], ["--delta-window", "6"]):
        with pytest.raises(ValueError, match="delta-order"):
            make_feat.main(["--conf", "x", "--wav-scp", "y", "--out-dir", "z"] + bad)
