"""SpecAugment on the HIP kernel (ctcn_spec_augment) through ops.spec_augment, utils/features.SpecAugment, utils/data_loader.DeviceContext
and steps/train_ctc.main.  The demand is bit-identity with the host twin (ctcn_spec_augment_host) and with the numpy restatement of the
contract (tests/spec_augment_ref.py): the draws are integer arithmetic, the warp's float64 operations are rounded one by one.

Shapes: B = 3, Tmax = 37, F = 5 with frames [37, 0, 11] -- an odd width, an empty utterance, one too short to warp at W = 6, two row tiles
with a ragged last one -- and B = 2, Tmax = 70, F = 81 with frames [70, 23]: the recipe's width, three row tiles.  Input rows at or beyond
an utterance's length hold NaN and the output is pre-filled with NaN where the entry point is called directly: a read past the length
or an element left unwritten shows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_context_ref as FR  # noqa: E402
import spec_augment_ref as SR  # noqa: E402
from ctc_pytorch_amd import _lib, ops  # noqa: E402
from ctc_pytorch_amd.utils import data_loader as DL  # noqa: E402
from ctc_pytorch_amd.utils import features  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 5
SMALL = dict(warp_window=6, num_freq_masks=1, freq_width=3, num_time_masks=1, time_width=8, time_ratio=0.5, fill=0.75)
WIDE = dict(warp_window=6, num_freq_masks=2, freq_width=15, num_time_masks=2, time_width=12, time_ratio=0.5, fill=-1.5)
SHAPES = {"small": (37, 5, [37, 0, 11], SMALL), "wide": (70, 81, [70, 23], WIDE)}
_BATCHES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ragged(name):
    """(padded batch with NaN behind every utterance, frame counts, the utterances, options), computed once per shape."""
    if name not in _BATCHES:
        Tmax, F, frames, kw = SHAPES[name]
        rs = np.random.RandomState(Tmax * 100 + F)
        batch = np.full((len(frames), Tmax, F), np.nan, dtype=np.float32)
        utts = []
        for b, T in enumerate(frames):
            x = rs.randn(T, F).astype(np.float32) * (10.0 ** rs.randint(-4, 5, size=(T, 1))).astype(np.float32)
            batch[b, :T] = x
            utts.append(x)
        _BATCHES[name] = (batch, frames, utts, kw)
    return _BATCHES[name]


def run_raw(batch, frames, dev, seed, utt_offset, kw):
    """ctcn_spec_augment called directly, the output pre-filled with NaN."""
    B, Tmax, F = batch.shape
    o = _lib.SpecAugOpts(**dict(SR.options(), **kw))
    x = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    out = torch.full((B, Tmax, F), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ctcn_spec_augment(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(fr.data_ptr()), ctypes.byref(o), seed, utt_offset,
                                            ctypes.c_void_p(out.data_ptr()), B, Tmax, F, _lib.stream_ptr()), "spec_augment")
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_is_the_host_twin_bit_for_bit(name, dev):
    batch, frames, utts, kw = ragged(name)
    offset = 3
    got = run_raw(batch, frames, dev, SEED, offset, kw)
    # rows at or beyond an utterance's length were never read (they hold NaN) and are zeros; every element was written
    assert not np.isnan(got).any()
    for b, T in enumerate(frames):
        assert not got[b, T:].any()
        twin = ops.spec_augment_host(utts[b], SEED, offset + b, **kw)
        assert np.array_equal(bits(got[b, :T]), bits(twin)), (b, int((bits(got[b, :T]) != bits(twin)).sum()))
    assert np.array_equal(bits(got), bits(SR.augment_batch(utts, SEED, offset, Tmax=batch.shape[1], **kw)))
    # the cases the shapes are there for did occur
    plans = [SR.plan(T, batch.shape[2], SEED, offset + b, **kw) for b, T in enumerate(frames)]
    assert plans[0]["warp"] is not None and (plans[-1]["warp"] is None) == (frames[-1] <= 12)
    assert any(n > 0 for p in plans for _, n in p["freq"]) and any(n > 0 for p in plans for _, n in p["time"])
    # the public op and the class: the same bits, from a list and from a device tensor of frame counts
    x = torch.from_numpy(batch).to(dev)
    aug = features.SpecAugment(seed=SEED, start_index=offset, **kw)
    for fr in (frames, torch.tensor(frames, dtype=torch.int32, device=dev)):
        out = ops.spec_augment(x, fr, SEED, offset, **kw)
        assert out.is_cuda and out.data_ptr() != x.data_ptr() and np.array_equal(bits(out.cpu().numpy()), bits(got))
    assert np.array_equal(bits(aug(x, frames).cpu().numpy()), bits(got)) and aug.index == offset + len(frames)
    assert not np.array_equal(bits(aug(x, frames).cpu().numpy()), bits(got)) and aug.index == offset + 2 * len(frames)   # the next draws
    assert np.array_equal(bits(aug(x, frames, utt_offset=offset).cpu().numpy()), bits(got)) and aug.index == offset + 2 * len(frames)


def test_all_parts_off_is_the_identity(dev):
    batch, frames, utts, _ = ragged("small")
    got = run_raw(batch, frames, dev, SEED, 0, {})
    for b, T in enumerate(frames):
        assert np.array_equal(bits(got[b, :T]), bits(utts[b])) and not got[b, T:].any() and not np.isnan(got[b]).any()


def test_an_utterance_does_not_depend_on_its_batch(dev):
    batch, frames, utts, kw = ragged("wide")
    in_batch = run_raw(batch, frames, dev, SEED, 0, kw)
    alone = run_raw(utts[1][None], [23], dev, SEED, 1, kw)               # B = 1, Tmax = 23, utt_offset = 1
    assert np.array_equal(bits(alone[0]), bits(in_batch[1, :23]))


def test_non_contiguous_features(dev):
    batch, frames, utts, kw = ragged("wide")
    clean = np.nan_to_num(batch, nan=0.5)
    x = torch.from_numpy(clean).to(dev)
    want = ops.spec_augment(x, frames, SEED, 0, **kw)
    strided = torch.from_numpy(np.ascontiguousarray(clean.transpose(0, 2, 1))).to(dev).transpose(1, 2)         # (B, Tmax, F) over (B, F, Tmax) memory
    wider = torch.zeros((2, 70, 90), device=dev)
    wider[:, :, 4:85] = x
    assert not strided.is_contiguous() and not wider[:, :, 4:85].is_contiguous()
    assert torch.equal(ops.spec_augment(strided, frames, SEED, 0, **kw), want)
    assert torch.equal(ops.spec_augment(wider[:, :, 4:85], frames, SEED, 0, **kw), want)


class _Base(torch.utils.data.Dataset):
    """Three utterances of base features in memory, as SpeechDataset(base_features=True) hands them on."""
    base_features = True

    def __init__(self, utts):
        self.utts = utts

    def __len__(self):
        return len(self.utts)

    def __getitem__(self, i):
        return torch.from_numpy(self.utts[i]), torch.LongTensor([1 + i, 2]), "utt%d" % i


def test_device_context_augments_the_base_batch(dev):
    rs = np.random.RandomState(12)
    utts = [rs.randn(T, 4).astype(np.float32) for T in (29, 14, 33)]
    kw = dict(warp_window=5, num_freq_masks=1, freq_width=2, num_time_masks=1, time_width=6, time_ratio=0.5, fill=-3.0)
    ctx = (1, 1, 2, 2)
    loader = DL.BaseFeatureLoader(_Base(utts), batch_size=2, shuffle=False)
    plain = [b for b in DL.DeviceContext(loader, dev, features.FrameContext(*ctx))]
    staged = DL.DeviceContext(loader, dev, features.FrameContext(*ctx), augment=features.SpecAugment(seed=SEED, **kw))
    epochs = [[b for b in staged] for _ in range(2)]
    seen = 0
    for epoch in epochs:
        assert len(epoch) == 2
        for k, got in enumerate(epoch):
            mine = utts[2 * k:2 * k + 2]
            want, want_frac, _ = FR.host_batch([SR.augment(u, SEED, seen + b, **kw) for b, u in enumerate(mine)], *ctx)
            assert np.array_equal(bits(got[0].cpu().numpy()), bits(want)) and np.array_equal(bits(got[1].cpu().numpy()), bits(want_frac))
            assert torch.equal(got[2], plain[k][2]) and torch.equal(got[3], plain[k][3]) and got[4] == plain[k][4]
            seen += len(mine)                                            # counted across batches AND epochs
    assert not torch.equal(epochs[0][0][0], epochs[1][0][0])             # a second epoch draws new masks
    # augment=None: the batches of today (the host loader path over the unaugmented utterances), epoch after epoch
    for again in (plain, [b for b in DL.DeviceContext(loader, dev, features.FrameContext(*ctx), augment=None)]):
        for k, got in enumerate(again):
            want, want_frac, _ = FR.host_batch(utts[2 * k:2 * k + 2], *ctx)
            assert np.array_equal(bits(got[0].cpu().numpy()), bits(want)) and np.array_equal(bits(got[1].cpu().numpy()), bits(want_frac))
    # data-parallel shards: two ranks augment a global batch exactly as one process does
    from ctc_pytorch_amd import parallel
    for rank in (0, 1):
        sharded = DL.DeviceContext(parallel.ShardedBatches(loader, rank, 2, log=lambda *_: None), dev, features.FrameContext(*ctx),
                                   augment=features.SpecAugment(seed=SEED, **kw))
        got = [b for b in sharded]
        assert len(got) == 1 and got[0][5] == 2                          # (the one-utterance batch is dropped: fewer utterances than ranks)
        assert torch.equal(got[0][0], epochs[0][0][0][rank:rank + 1])


def _toy_corpus(d):
    """The corpus of test_gpu_kernels.test_end_to_end_train_checkpoint_decode: 24 utterances of 8 noisy 40-column prototypes."""
    rs = np.random.RandomState(7)
    phones = ["p%d" % i for i in range(8)]
    proto = rs.standard_normal((len(phones), 40)).astype(np.float32) * 2.0
    mats, labs = {}, {}
    for u in range(24):
        seq = [int(k) for k in rs.randint(0, len(phones), size=int(rs.randint(4, 8)))]
        frames = [proto[k] + 0.3 * rs.standard_normal(40) for k in seq for _ in range(int(rs.randint(5, 9)))]
        mats["utt%02d" % u] = np.asarray(frames, dtype=np.float32)
        labs["utt%02d" % u] = " ".join(phones[k] for k in seq)
    DL.write_kaldi_ark(d + "/feats.ark", d + "/feats.scp", mats)
    open(d + "/text", "w").write("".join("%s %s\n" % kv for kv in labs.items()))
    open(d + "/vocab", "w").write("".join("%d %s\n" % (i, ph) for i, ph in enumerate(phones)))


def test_toy_corpus_trains_with_the_driver_key(dev, tmp_path):
    """Two training steps (24 utterances in batches of 12) and one dev pass of steps/train_ctc.main.  With a real learning rate the
    augmented run's loss is finite.  With the weights frozen (learning rate 0, no BatchNorm: no running statistics either) the key-on and
    key-off runs hold identical weights at the dev pass: their dev losses are equal -- the dev loader never augments -- while their first
    training losses differ."""
    from ctc_pytorch_amd.steps import train_ctc
    d = str(tmp_path)
    _toy_corpus(d)

    def run(on, lr, batch_norm):
        conf = dict(vocab_file=d + "/vocab", train_scp_path=d + "/feats.scp", train_lab_path=d + "/text", valid_scp_path=d + "/feats.scp",
                    valid_lab_path=d + "/text", left_ctx=0, right_ctx=0, n_skip_frame=1, n_downsample=1, batch_size=12, shuffle_train=False,
                    num_workers=0, rnn_input_size=40, rnn_hidden_size=32, rnn_layers=2, rnn_type="nn.LSTM", bidirectional=True,
                    batch_norm=batch_norm, add_cnn=False, layers=2, channel="[(1,32),(32,32)]", kernel_size="[(3,3),(3,3)]",
                    stride="[(1,2),(2,2)]", padding="[(1,1),(1,1)]", pooling="None", activation_function="relu", drop_out=0.0, init_lr=lr,
                    weight_decay=0.0, end_adjust_acc=2.0, lr_decay=0.5, num_epoches=1, verbose_step=1, seed=1, device_context=True)
        if on:
            conf["spec_augment"] = True
        lines = []
        _, hist = train_ctc.main(conf, log=lines.append)
        steps = [float(l.split("cur_loss = ")[1].split(",")[0]) for l in lines if isinstance(l, str) and "cur_loss" in l]
        assert len(steps) == 2 and len(hist["loss"]) == 1
        return steps, hist

    steps, hist = run(True, 1e-2, True)
    assert np.isfinite(steps).all() and np.isfinite(hist["loss"]).all() and np.isfinite(hist["dev_loss"]).all()
    (on_steps, on_hist), (off_steps, off_hist) = run(True, 0.0, False), run(False, 0.0, False)
    assert np.isfinite(on_steps).all() and np.isfinite(off_steps).all()
    assert on_steps[0] != off_steps[0] and on_hist["loss"] != off_hist["loss"]
    assert on_hist["dev_loss"] == off_hist["dev_loss"] and on_hist["dev_acc"] == off_hist["dev_acc"]
    with pytest.raises(ValueError, match="spec_augment.*device_context"):
        train_ctc.main(dict(seed=1, spec_augment=True), log=lambda *_: None)
