"""Deltas, splice, skip and downsample pad on the HIP kernel (ctcn_frame_context) through its C entry point, ops.frame_context,
utils/features.FrameContext and utils/data_loader.DeviceContext.  The demand is bit-identity throughout: without deltas the kernel copies,
and the yardstick is the host loader path (tests/frame_context_ref.host_batch: make_context, skip_feat, the pad of
SpeechDataset.__getitem__, create_input); with deltas every element is the ascending float64 sum of exact products rounded once, one
number on any machine (include/ctcn.h), and the yardsticks are the numpy restatement and the host twin.

Shapes: B = 5 with frames [0, 1, 2, 7, Tin_max], Tin_max one frame more than the base frames behind one workgroup's tile of output rows, so
the longest utterance crosses a tile boundary with context reaching into both tiles and the short ones are shorter than the context, the
delta reach and the skip.  Base rows at or beyond an utterance's length hold NaN and the outputs are pre-filled with NaN: a read past the
length or an element left unwritten shows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_context_ref as FR  # noqa: E402
from ctc_pytorch_amd import _lib, nn, ops  # noqa: E402
from ctc_pytorch_amd.testing import synth  # noqa: E402
from ctc_pytorch_amd.utils import data_loader as DL  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

pytestmark = pytest.mark.gpu
SETTINGS = FR.SETTINGS
_BATCHES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tile_span(F, left, right, skip, nd, order=0, window=2):
    """Delta'd frames behind one full tile of output rows: (rows - 1) skip + left + 1 + right."""
    rows = ops.frame_context_tile(F, left, right, skip, nd, order, window)
    return (rows - 1) * max(skip, 1) + left + 1 + right


def ragged(F, Tin_max):
    """(padded batch with NaN behind every utterance, frame counts, the utterances), computed once per shape."""
    key = (F, Tin_max)
    if key not in _BATCHES:
        rs = np.random.RandomState(1000 * F + Tin_max)
        frames = [0, 1, 2, 7, Tin_max]
        batch = np.full((len(frames), Tin_max, F), np.nan, dtype=np.float32)
        utts = []
        for b, T in enumerate(frames):
            batch[b, :T] = rs.randn(T, F).astype(np.float32)
            utts.append(batch[b, :T].copy())
        _BATCHES[key] = (batch, frames, utts)
    return _BATCHES[key]


def run_raw(batch, frames, dev, left=0, right=0, skip=1, nd=1, order=0, window=2):
    """ctcn_frame_context called directly, every output pre-filled with NaN: (out, out_frames, fractions) as numpy arrays."""
    B, Tin_max, F = batch.shape
    opts = _lib.ContextOpts(left=left, right=right, skip=skip, n_downsample=nd, delta_order=order, delta_window=window)
    Tout_max = ops.context_frames(Tin_max, skip, nd)
    x = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    out = torch.full((B, Tout_max, (left + 1 + right) * F * (order + 1)), float("nan"), dtype=torch.float32, device=dev)
    out_frames = torch.full((B,), -7, dtype=torch.int32, device=dev)
    fractions = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ctcn_frame_context(p(x), p(fr), ctypes.byref(opts), p(out), p(out_frames), p(fractions), B, Tin_max, F, Tout_max,
                                             _lib.stream_ptr()), "frame_context")
    return out.cpu().numpy(), out_frames.cpu().numpy(), fractions.cpu().numpy()


def check_against_host(got, utts, Tin_max, left, right, skip, nd):
    out, out_frames, fractions = got
    want, want_frac, want_frames = FR.host_batch(utts, left, right, skip, nd, pad_to=Tin_max)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(fractions)), "an element left unwritten, or a row past an utterance's length read"
    assert out.shape == want.shape and np.array_equal(out_frames, want_frames)
    assert np.array_equal(bits(out), bits(want)), int((bits(out) != bits(want)).sum())
    assert np.array_equal(bits(fractions), bits(want_frac)), (fractions, want_frac)


@pytest.mark.parametrize("F", [1, 13, 81])
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "l%d_r%d_s%d_d%d" % s)
def test_ragged_batch_is_the_host_loader_bit_for_bit(setting, F, dev):
    left, right, skip, nd = setting
    Tin_max = tile_span(F, left, right, skip, nd) + 1
    batch, frames, utts = ragged(F, Tin_max)
    check_against_host(run_raw(batch, frames, dev, left, right, skip, nd), utts, Tin_max, left, right, skip, nd)
    # the public op: the same bits, from a list and from a device tensor of frame counts
    x = torch.from_numpy(batch).to(dev)
    for fr in (frames, torch.tensor(frames, dtype=torch.int32, device=dev), torch.tensor(frames, device=dev)):
        out, out_frames, fractions = ops.frame_context(x, fr, left, right, skip, nd)
        assert out.is_cuda and out_frames.dtype == torch.int32 and fractions.dtype == torch.float32
        check_against_host((out.cpu().numpy(), out_frames.cpu().numpy(), fractions.cpu().numpy()), utts, Tin_max, left, right, skip, nd)


def delta_reference(utts, order, window, ctx, Tin_max):
    """The float64 restatement of every utterance, then the host loader path over it; the same through the host twin."""
    left, right, skip, nd = ctx
    want = FR.host_batch([FR.deltas64(u, order, window) for u in utts], left, right, skip, nd, pad_to=Tin_max)
    rows = want[0].shape[1]
    twin = [FR.host_twin(u, left, right, skip, nd, order, window, out_rows=rows) for u in utts]
    return want, twin


def check_deltas(F, order, window, ctx, dev):
    left, right, skip, nd = ctx
    Tin_max = tile_span(F, left, right, skip, nd, order, window) + 1
    batch, frames, utts = ragged(F, Tin_max)
    out, out_frames, fractions = run_raw(batch, frames, dev, left, right, skip, nd, order, window)
    (want, want_frac, want_frames), twin = delta_reference(utts, order, window, ctx, Tin_max)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(fractions))
    assert out.shape == want.shape and np.array_equal(out_frames, want_frames) and np.array_equal(bits(fractions), bits(want_frac))
    assert np.array_equal(bits(out), bits(want)), int((bits(out) != bits(want)).sum())
    for b, (t_out, t_n, t_frac) in enumerate(twin):
        assert t_n == out_frames[b] and np.array_equal(bits(out[b]), bits(t_out)) and np.float32(fractions[b]) == np.float32(t_frac)
    return out, utts


@pytest.mark.parametrize("F", [1, 13, 81])
@pytest.mark.parametrize("order,window", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_deltas_are_the_float64_restatement_and_the_host_twin(order, window, F, dev):
    out, utts = check_deltas(F, order, window, (0, 0, 1, 1), dev)
    # and within the float32 worst case of Kaldi's own sequential form
    for b, u in enumerate(utts):
        k32, bound = FR.deltas_kaldi32(u, order, window)
        assert np.all(np.abs(out[b, :u.shape[0]].astype(np.float64) - k32) <= bound)


@pytest.mark.parametrize("ctx", [(0, 2, 2, 2), (2, 1, 3, 4)], ids=["shipped", "l2_r1_s3_d4"])
def test_deltas_then_splice_then_skip(ctx, dev):
    check_deltas(13, 2, 2, ctx, dev)


def test_wide_rows(dev):
    """F = 257 (the spectrogram's) with two delta orders: 771 columns a frame, the tile shrinks to fit the LDS."""
    assert ops.frame_context_tile(257, delta_order=2) < 16
    check_deltas(257, 2, 2, (0, 0, 1, 1), dev)
    check_deltas(257, 2, 5, (1, 1, 2, 2), dev)


def test_recipe_batch(dev):
    """The shipped configuration at the shipped batch size: 8 x 800 x 81 -> 8 x 400 x 243, fifty tiles an utterance."""
    rs = np.random.RandomState(8)
    frames = [800, 799, 641, 640, 333, 17, 1, 0]
    batch = np.full((8, 800, 81), np.nan, dtype=np.float32)
    utts = []
    for b, T in enumerate(frames):
        batch[b, :T] = rs.randn(T, 81).astype(np.float32)
        utts.append(batch[b, :T].copy())
    check_against_host(run_raw(batch, frames, dev, 0, 2, 2, 2), utts, 800, 0, 2, 2, 2)


def test_contracts(dev):
    F, (left, right, skip, nd) = 13, (0, 2, 2, 2)
    Tin_max = tile_span(F, left, right, skip, nd) + 1
    batch, frames, utts = ragged(F, Tin_max)
    # a frame count above Tin_max is clamped (and a negative one counts as 0)
    x = torch.from_numpy(np.nan_to_num(batch[3:], nan=0.25)).to(dev)
    out, out_frames, fractions = ops.frame_context(x, [Tin_max + 9, Tin_max], left, right, skip, nd)
    full = ops.frame_context(x[:1], [Tin_max], left, right, skip, nd)
    assert torch.equal(out[0], full[0][0]) and out_frames.tolist() == [ops.context_frames(Tin_max, skip, nd)] * 2 and fractions.tolist() == [1.0, 1.0]
    out, out_frames, fractions = ops.frame_context(x, [-3, Tin_max], left, right, skip, nd)
    assert out_frames.tolist()[0] == 0 and fractions.tolist()[0] == 0.0 and not out[0].any()
    # device tensors only
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_context(x.cpu(), [Tin_max, Tin_max])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_context(x, torch.tensor([Tin_max, Tin_max]))
    # options outside the limits raise before any launch; shapes and types that are not the contract's raise too
    for kw in (dict(left=65), dict(skip=1025), dict(delta_order=3), dict(delta_window=6), dict(delta_order=1, delta_window=0), dict(n_downsample=0)):
        with pytest.raises(RuntimeError, match="rc=-[13]"):
            ops.frame_context(x, [Tin_max, Tin_max], **kw)
    with pytest.raises(ValueError):
        ops.frame_context(x, [Tin_max])
    with pytest.raises(ValueError):
        ops.frame_context(x[0], [Tin_max])
    with pytest.raises(TypeError):
        ops.frame_context(x.double(), [Tin_max, Tin_max])
    # an empty time axis: nothing to launch over, the vectors are still written
    out, out_frames, fractions = ops.frame_context(torch.zeros((2, 0, F), device=dev), [0, 0], left, right, skip, nd)
    assert tuple(out.shape) == (2, 0, 3 * F) and out_frames.tolist() == [0, 0] and fractions.tolist() == [0.0, 0.0]


def test_fbank_to_context_to_model(dev):
    """Fbank -> FrameContext -> CTC_Model.forward on one device, nothing on the host in between; the spliced batch is what the host path
    makes of the same filterbank output."""
    cfg = features.FbankConfig(num_mel_bins=80, use_energy=True, dither=0.0)           # 81 columns, the recipe's
    fb = features.Fbank(cfg, dev)
    feats, frames = fb(synth.make_waves(5, [16000 * 3 // 10, 16000 * 2 // 10 + 77]))
    ctx = features.FrameContext(0, 2, 2, 2)
    x, out_frames, fractions = ctx(feats, frames)
    assert x.is_cuda and ctx.out_dim(fb.feat_dim) == 243 and tuple(x.shape) == (2, ctx.out_frames(feats.shape[1]), 243)
    host, n = feats.cpu().numpy(), frames.cpu().numpy()
    want, want_frac, want_frames = FR.host_batch([host[b, :n[b]] for b in range(2)], 0, 2, 2, 2)
    assert np.array_equal(bits(x.cpu().numpy()), bits(want)) and np.array_equal(bits(fractions.cpu().numpy()), bits(want_frac))
    assert np.array_equal(out_frames.cpu().numpy(), want_frames)
    from ctc_pytorch_amd.models.model_ctc import CTC_Model
    rp = {"rnn_input_size": 243, "rnn_hidden_size": 16, "rnn_layers": 2, "rnn_type": nn.LSTM, "bidirectional": True, "batch_norm": True}
    model = CTC_Model(rnn_param=rp, num_class=10, drop_out=0.0).to(dev).eval()
    with torch.no_grad():
        lp = model(x)
    assert tuple(lp.shape) == (x.shape[1], 2, 10) and bool(torch.isfinite(lp).all())


class _Opts(object):
    left_ctx, right_ctx, n_skip_frame, n_downsample = 0, 2, 2, 2


def test_device_context_loader_equals_the_host_loader(tmp_path, dev):
    rs = np.random.RandomState(3)
    lengths = [37, 5, 64, 1, 23, 48]
    mats = {"utt%d" % i: rs.randn(T, 7).astype(np.float32) for i, T in enumerate(lengths)}
    ark, scp, lab, units = (str(tmp_path / n) for n in ("feats.ark", "feats.scp", "text", "units"))
    DL.write_kaldi_ark(ark, scp, mats)
    with open(units, "w") as f:
        f.write("a\nb\nc\n")
    with open(lab, "w") as f:
        for i, utt in enumerate(mats):
            f.write("%s %s\n" % (utt, " ".join("abc"[(i + k) % 3] for k in range(1 + i % 4))))
    vocab = DL.Vocab(units)
    host = list(DL.SpeechDataLoader(DL.SpeechDataset(vocab, scp, lab, _Opts), batch_size=4, shuffle=False))
    base = DL.BaseFeatureLoader(DL.SpeechDataset(vocab, scp, lab, _Opts, base_features=True), batch_size=4, shuffle=False)
    staged = DL.DeviceContext(base, dev, features.FrameContext(0, 2, 2, 2))
    assert len(staged) == len(host) == 2
    for epoch in range(2):                                             # the second pass reuses the pinned staging slots
        got = list(staged)
        assert len(got) == 2 and got[1][0].shape[0] == 2               # the last batch is short
        for g, h in zip(got, host):
            assert len(g) == 5 and all(t.is_cuda for t in g[:4])
            assert g[0].dtype == torch.float32 and g[1].dtype == torch.float32 and g[2].dtype == torch.int64 and g[3].dtype == torch.int64
            assert g[0].shape == h[0].shape and np.array_equal(bits(g[0].cpu().numpy()), bits(h[0].numpy()))
            assert np.array_equal(bits(g[1].cpu().numpy()), bits(h[1].numpy()))
            assert torch.equal(g[2].cpu(), h[2]) and torch.equal(g[3].cpu(), h[3]) and g[4] == h[4]
    # the host prefetcher over the host loader yields the same batches: the two paths are interchangeable in the training loop
    for g, h in zip(DL.DevicePrefetcher(DL.SpeechDataLoader(DL.SpeechDataset(vocab, scp, lab, _Opts), batch_size=4, shuffle=False), dev), got):
        assert all(torch.equal(a, b) for a, b in zip(g[:4], h[:4])) and g[4] == h[4]
    # a data-parallel shard: padded to the global T_max, so its rows and fractions are the global batch's, and the 6th entry rides along
    from ctc_pytorch_amd import parallel
    for rank in (0, 1):
        for g, h in zip(DL.DeviceContext(parallel.ShardedBatches(base, rank, 2), dev, features.FrameContext(0, 2, 2, 2)), host):
            lo, hi = parallel.shard_range(h[0].shape[0], rank, 2)
            assert len(g) == 6 and g[5] == h[0].shape[0] and g[4] == h[4][lo:hi]
            assert np.array_equal(bits(g[0].cpu().numpy()), bits(h[0][lo:hi].numpy())) and np.array_equal(bits(g[1].cpu().numpy()), bits(h[1][lo:hi].numpy()))
            assert torch.equal(g[2].cpu(), h[2][lo:hi]) and torch.equal(g[3].cpu(), h[3][lo:hi])
    with pytest.raises(TypeError, match="int32 frame counts"):
        next(iter(DL.DeviceContext(DL.SpeechDataLoader(DL.SpeechDataset(vocab, scp, lab, _Opts), batch_size=4), dev, features.FrameContext(0, 2, 2, 2))))


def test_make_feat_delta_options(tmp_path, dev):
    """make_feat.py --delta-order 2: the archive holds [static | delta | delta-delta] of the normalised MFCCs, 13 -> 39 columns."""
    import wave
    from ctc_pytorch_amd.steps import make_feat
    waves = synth.make_waves(9, [4000, 2400])
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for i, w in enumerate(waves):
            path = tmp_path / ("w%d.wav" % i)
            with wave.open(str(path), "wb") as wf:
                wf.setnchannels(1)
                wf.setsampwidth(2)
                wf.setframerate(16000)
                wf.writeframes(np.round(w).astype("<i2").tobytes())
            f.write("utt%d %s\n" % (i, path))
    conf = tmp_path / "mfcc.conf"
    conf.write_text("--dither=0\n--use-energy=false\n")
    common = ["--conf", str(conf), "--feat-type", "mfcc", "--wav-scp", str(scp), "--compute-cmvn", "--device", str(dev)]
    _, base_scp = make_feat.main(common + ["--out-dir", str(tmp_path / "base")], log=lambda *_: None)
    _, delta_scp = make_feat.main(common + ["--out-dir", str(tmp_path / "deltas"), "--delta-order", "2"], log=lambda *_: None)
    read = lambda path: [DL.read_kaldi_matrix(line.split()[1]) for line in open(path)]
    for b, d in zip(read(base_scp), read(delta_scp)):
        assert b.shape[1] == 13 and d.shape == (b.shape[0], 39)
        assert np.array_equal(bits(d), bits(FR.deltas64(b, 2, 2)))
    assert open(tmp_path / "base" / "global_mfcc_cmvn.txt").read() == open(tmp_path / "deltas" / "global_mfcc_cmvn.txt").read()


def test_drivers_with_device_context_are_the_host_loaders_runs(tmp_path, dev):
    """steps/train_ctc.main and steps/decode_ctc.main over one small archive with `device_context` off and on: the batches are the same bits,
    so the loss history, the parameters and the error rates are the same numbers."""
    from ctc_pytorch_amd.steps import decode_ctc, train_ctc
    rs = np.random.RandomState(21)
    mats = {"utt%d" % i: rs.randn(T, 7).astype(np.float32) for i, T in enumerate([41, 30, 57, 12, 36, 49])}
    ark, scp, lab, units = (str(tmp_path / n) for n in ("feats.ark", "feats.scp", "text", "units"))
    DL.write_kaldi_ark(ark, scp, mats)
    with open(units, "w") as f:
        f.write("a\nb\nc\n")
    with open(lab, "w") as f:
        for i, utt in enumerate(mats):
            f.write("%s %s\n" % (utt, " ".join("abc"[(i + k) % 3] for k in range(2 + i % 3))))
    runs = {}
    for on in (False, True):
        conf = dict(vocab_file=units, train_scp_path=scp, train_lab_path=lab, valid_scp_path=scp, valid_lab_path=lab, test_scp_path=scp,
                    test_lab_path=lab, left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2, batch_size=4, shuffle_train=False,
                    num_workers=0, rnn_input_size=21, rnn_hidden_size=16, rnn_layers=2, rnn_type="nn.LSTM", bidirectional=True,
                    batch_norm=True, add_cnn=False, layers=2, channel="[(1,32),(32,32)]", kernel_size="[(3,3),(3,3)]", stride="[(1,2),(2,2)]",
                    padding="[(1,1),(1,1)]", pooling="None", activation_function="relu", drop_out=0.0, init_lr=1e-2, weight_decay=0.0,
                    end_adjust_acc=2.0, lr_decay=0.5, num_epoches=2, verbose_step=100, seed=1, checkpoint_dir=str(tmp_path / ("ckpt%d" % on)),
                    exp_name="toy", decode_type="Greedy", use_gpu=True)
        if on:
            conf["device_context"] = True
        model, hist = train_ctc.main(conf, log=lambda *_: None)
        flat = torch.cat([q.detach().reshape(-1) for q in model.parameters()]).cpu()
        runs[on] = (hist, flat, decode_ctc.main(conf, log=lambda *_: None))
    assert runs[True][0] == runs[False][0] and torch.equal(runs[True][1], runs[False][1]) and runs[True][2] == runs[False][2]
    assert np.isfinite(runs[True][0]["loss"]).all() and len(runs[True][0]["loss"]) == 2
