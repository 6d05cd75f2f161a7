"""Decode + score with the utterance lengths passed to the model: steps/test_ctc.py's loop, made length-aware from outside.

    python -m ctc_pytorch_amd.steps.decode_ctc --conf conf/ctc_config.yaml [--mask-padding]
    torchrun --nproc_per_node=8 -m ctc_pytorch_amd.steps.decode_ctc --conf ...        (replicas-only sharded decode, as test_ctc.py)

Same YAML as steps/test_ctc.py plus the key `mask_padding` (default false: this IS test_ctc.main).  With the key on, the decode loop, the
three-stream search pipeline, the scoring and the sharding are still test_ctc.decode_and_score[_sharded] -- there is no second copy of them.
`length_aware(model, loader)` hands that loop
  * a model whose call passes CTC_Model.forward(input_lengths=): the frames ride on the input tensor of their batch (`_Batch`), recovered from
    the loader's float32 fraction with steps/train_ctc.input_frames_from_fraction (round to nearest), so an utterance's posteriors do not
    depend on what shares its minibatch;
  * a loader whose length fractions are restated on the OUTPUT time axis, (model.output_lengths(frames) + 0.5) / T_out: the loop's
    floor(fraction * T_out) then is exactly model.output_lengths(frames), the frames the decoders have to see.
Checkpoints are the same files.

Keys `error_report`, `score_map`, `score_map_cols` (--error-report, --score-map, --score-map-cols; default off): the error breakdown behind the
word error rate.  The loop is still test_ctc's: it is handed `_ScoringDecoder`, a proxy of the decoder whose `wer` returns what the decoder's
own returns and, on the side, aligns the two strings' word ids (folded by the score map) in the library's host code and tallies the
alignment into a utils.scoring.ErrorStats.  The CER / WER lines and the return value do not change; the report is logged after them.

Keys `ctm` (--ctm PATH; default off) and `ctm_frame_shift` (--ctm-frame-shift; seconds per model INPUT frame as the feature extraction made
them, default 0.01): a NIST CTM file of what was recognised -- per token its start, duration and confidence (Decoder.decode_timed,
utils/ctm.py).  The loop is still test_ctc's: it is handed `_CtmDecoder`, a proxy that decodes every batch once, through `decode_timed`,
keeps the entries and hands the loop the strings put together from their tokens (the decoder's own join: the strings `decode` returns);
`_recorded` notes the loader's utterance ids in loader order, which is decode order.  A token's frames are output frames times `input_frames_per_output_frame(model)` (the front-end geometry
CTC_Model.output_lengths uses) times the loader's frame skip (`n_skip_frame`).  Under torchrun rank r writes PATH.r (its own minibatches).
The CER / WER lines and the return value do not change.

Key `device_context` (--device-context; default off): the test archive is read as BASE features and left_ctx / right_ctx / n_skip_frame /
n_downsample are applied on the GPU (utils/data_loader.DeviceContext: one launch per batch on the copy stream); the loop sees the batches the
host loader would have made, bit for bit.

Keys `rnnlm_path`, `rnnlm_weight` (0.5), `rnnlm_nbest` (10), `rnnlm_len_bonus` (0.0) (--rnnlm-path, --rnnlm-weight, --rnnlm-nbest,
--rnnlm-len-bonus; default off): n-best rescoring of a beam decode with an RNN language model (a package of steps/train_rnnlm.py): the search
returns its rnnlm_nbest best labellings, the LM scores them on the device and the hypothesis is the one with the largest
(search score + rnnlm_weight * ln P_lm) + rnnlm_len_bonus * length (utils/ctcDecoder.BeamDecoder).  The loop is still test_ctc's.  A Greedy
decode_type with rnnlm_path set is an error, not a silent plain decode.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from ctc_pytorch_amd.steps import test_ctc  # noqa: E402
from ctc_pytorch_amd.steps.train_ctc import device_context, epoch_options, input_frames_from_fraction, report_options  # noqa: E402


class _Batch(torch.Tensor):
    """The (B,T,F) inputs of one minibatch with the real frames of every utterance attached; `.to(device)` carries them over."""

    def to(self, *args, **kwargs):
        out = super().to(*args, **kwargs).as_subclass(_Batch)
        out.frames = self.frames
        return out


class _LengthAwareModel(torch.nn.Module):
    """model(inputs) -> model(inputs, input_lengths=frames of that batch); eval() / train() reach the wrapped model."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, inputs):
        return self.model(inputs.as_subclass(torch.Tensor), input_lengths=inputs.frames)


def output_fractions(out_len, t_out):
    """float32 fractions f with floor(float32(f * t_out)) == out_len: the centre of the frame count's unit interval (the rounding of the
    float32 product moves it by (n + 0.5) * 2^-23 at most, far from either end)."""
    return ((np.asarray(out_len, dtype=np.float64) + 0.5) / float(t_out)).astype(np.float32)


def _length_aware_batches(model, loader):
    for inputs, input_sizes, targets, target_sizes, utt_list in loader:
        t_in = int(inputs.shape[1])
        frames = torch.from_numpy(input_frames_from_fraction(input_sizes.cpu(), t_in))
        batch = inputs.as_subclass(_Batch)
        batch.frames = frames
        t_out = int(model.output_lengths([t_in])[0])
        frac = torch.from_numpy(output_fractions(model.output_lengths(frames).numpy(), t_out))
        yield batch, frac, targets, target_sizes, utt_list


def length_aware(model, loader):
    """(model, loader) for steps/test_ctc.decode_and_score[_sharded] with the utterance lengths passed to the model (module docstring)."""
    return _LengthAwareModel(model), _length_aware_batches(model, loader)


def _labels_on_host(loader):
    """A device-staged loader as the scoring loop reads it: inputs stay on the device, the length fractions and the labels (a few hundred
    bytes, which the loop turns into strings on the host) come back."""
    for batch in loader:
        yield (batch[0], batch[1].cpu(), batch[2].cpu(), batch[3].cpu()) + tuple(batch[4:])


class _ScoringDecoder(object):
    """The decoder, as test_ctc.decode_and_score sees it, with one addition: every `wer(hypothesis, label)` also tallies the alignment of
    the two word sequences into `stats`.  Everything else -- decode, decode_async, cer, the num_word / num_char counters the loop keeps on
    the decoder -- is the wrapped decoder's, read and written through."""

    def __init__(self, decoder, stats, index2word, class_map=None):
        items = index2word.items() if isinstance(index2word, dict) else enumerate(index2word)
        ids = {}
        for k, w in sorted((int(k), w) for k, w in items):
            ids.setdefault(w, k)
        object.__setattr__(self, "_decoder", decoder)
        object.__setattr__(self, "_score", (stats, ids, class_map))

    def __getattr__(self, name):
        return getattr(self._decoder, name)

    def __setattr__(self, name, value):
        setattr(self._decoder, name, value)

    def wer(self, s1, s2):
        from ctc_pytorch_amd.utils.scoring import align_ids
        stats, ids, class_map = self._score
        unknown = {}                                       # words outside the vocabulary: ids past it, never entered in the table
        word_id = lambda w: ids[w] if w in ids else unknown.setdefault(w, stats.V + len(unknown))
        counts, pairs = align_ids([word_id(w) for w in s1.split()], [word_id(w) for w in s2.split()], class_map)
        stats.add_pairs(counts, pairs)
        return self._decoder.wer(s1, s2)


def input_frames_per_output_frame(model):
    """Input frames one output frame of `model` advances by: the product of the time strides and time poolings of its convolutional
    front-end -- the numbers LayerCNN.out_lengths divides by -- and 1 without one."""
    stride = 1
    if getattr(model, "add_cnn", False):
        for block in model.conv:
            conv_s = block.conv.stride
            stride *= int(conv_s[0] if isinstance(conv_s, (tuple, list)) else conv_s)
            if block.pooling is not None:
                pool = block.pooling.kernel_size
                stride *= int(pool[0] if isinstance(pool, (tuple, list)) else pool)
    return stride


def _recorded(loader, seen):
    """The loader, with the utterance ids of every minibatch appended to `seen` as it goes by."""
    for batch in loader:
        seen.append(list(batch[4]))
        yield batch


class _CtmDecoder(object):
    """The decoder, as test_ctc.decode_and_score sees it, decoding every batch ONCE, through `decode_timed`: the entries go into `timed`
    (one list per call) and the strings the loop scores are put together from their tokens (Decoder.timed_strings: the decoder's own join),
    so a beam search does not run twice.  A batch with an utterance that has no entry (a search that ended with a status) is handed to
    the decoder's own `decode`, which raises what it raises without `ctm`.  `decode_async` is kept for the loop that asks for it; its
    result is ready when it returns (decode_timed ends with the copy to the host), so the batches are not overlapped while `ctm` is on.
    Everything else -- cer, wer, the num_word / num_char counters -- is the wrapped decoder's, read and written through."""

    def __init__(self, decoder, timed, frame_stride):
        object.__setattr__(self, "_decoder", decoder)
        object.__setattr__(self, "_ctm", (timed, frame_stride))

    def __getattr__(self, name):
        inner = getattr(self._decoder, name)
        if name != "decode_async":
            return inner

        def decode_async(probs, lens):
            strings = self.decode(probs, lens)
            return lambda: strings
        return decode_async

    def __setattr__(self, name, value):
        setattr(self._decoder, name, value)

    def decode(self, probs, lens):
        timed, frame_stride = self._ctm
        entries = self._decoder.decode_timed(probs, lens, frame_stride=frame_stride)
        timed.append(entries)
        if any(e is None for e in entries):
            return self._decoder.decode(probs, lens)
        return self._decoder.timed_strings(entries)


def write_ctm_file(path, seen, timed, frame_shift, rank=0, world=1):
    """The CTM file of one rank: call k of the decoder was minibatch rank + k * world of the loader (test_ctc.decode_and_score_sharded's
    deal).  PATH for one process, PATH.<rank> under torchrun.  Returns the file's name."""
    from ctc_pytorch_amd.utils.ctm import write_ctm
    name = path if world <= 1 else "%s.%d" % (path, rank)
    with open(name, "w") as fh:
        for k, entries in enumerate(timed):
            write_ctm(fh, seen[rank + k * world if world > 1 else k], entries, frame_shift=frame_shift)
    return name


def decode_and_score(model, loader, decoder, index2word, device, verbose=False, log=print, mask_padding=True, rank=0, world=1,
                     stats=None, class_map=None, ctm=None, ctm_frame_shift=0.01, n_skip_frame=1):
    """steps/test_ctc.decode_and_score_sharded (one process: decode_and_score) over the length-aware pair; mask_padding=False: over the
    plain one.  stats (a host utils.scoring.ErrorStats): the loop scores through _ScoringDecoder, the stats are summed over the ranks
    beside the four totals, and rank 0 logs the report after the CER / WER lines.  ctm (a file name): the timed tokens of every utterance
    go to that file (module docstring), in seconds of ctm_frame_shift per input frame; n_skip_frame: the loader's frame skip."""
    seen, timed = [], []
    if ctm:
        stride = input_frames_per_output_frame(model) * max(int(n_skip_frame or 1), 1)
        loader, decoder = _recorded(loader, seen), _CtmDecoder(decoder, timed, stride)
    if mask_padding:
        model, loader = length_aware(model, loader)
    if stats is None:
        out = test_ctc.decode_and_score_sharded(model, loader, decoder, index2word, device, rank, world, verbose=verbose, log=log)
        if ctm:
            write_ctm_file(ctm, seen, timed, float(ctm_frame_shift), rank, world)
        return out
    out = test_ctc.decode_and_score_sharded(model, loader, _ScoringDecoder(decoder, stats, index2word, class_map), index2word, device, rank,
                                            world, verbose=verbose, log=log)
    if ctm:
        write_ctm_file(ctm, seen, timed, float(ctm_frame_shift), rank, world)
    if world > 1:
        import torch.distributed as dist
        t = stats.state().to(device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        stats._state.copy_(t)
    if rank == 0:
        log(stats.report())
    return out


def ctm_options(opts):
    """The keys `ctm` / `ctm_frame_shift` of a Config as decode_and_score's keyword arguments; {} while `ctm` is off (the default)."""
    path = getattr(opts, "ctm", None)
    if not path:
        return {}
    return {"ctm": str(path), "ctm_frame_shift": float(getattr(opts, "ctm_frame_shift", 0.01))}


def lm_order_option(opts):
    """The key `lm_order` of a Config: 2 (the default: the reference's bigram search) or 3 (the ARPA file's \\3-grams: section is used)."""
    order = int(getattr(opts, "lm_order", 2) or 2)
    if order not in (2, 3):
        raise ValueError("lm_order must be 2 or 3, got %r" % (order,))
    return order


def rnnlm_options(opts):
    """The keys `rnnlm_path` / `rnnlm_weight` / `rnnlm_nbest` / `rnnlm_len_bonus` of a Config as BeamDecoder's keyword arguments; {} while
    `rnnlm_path` is off (the default)."""
    path = getattr(opts, "rnnlm_path", None)
    if not path:
        return {}
    nbest = int(getattr(opts, "rnnlm_nbest", 10))
    if nbest < 1:
        raise ValueError("rnnlm_nbest must be at least 1, got %d" % nbest)
    return {"rnnlm": str(path), "rnnlm_weight": float(getattr(opts, "rnnlm_weight", 0.5)), "rnnlm_nbest": nbest,
            "rnnlm_len_bonus": float(getattr(opts, "rnnlm_len_bonus", 0.0))}


def make_decoder(opts, index2word):
    """test_ctc.make_decoder; with lm_order 3 and a beam decode_type the BeamDecoder is built with a trigram LM, with rnnlm_path with an
    RNN LM that rescores its n-best list."""
    order = lm_order_option(opts)
    rnnlm = rnnlm_options(opts)
    if rnnlm and opts.decode_type == "Greedy":
        raise ValueError("rnnlm_path rescores a beam search's n-best list: decode_type must not be Greedy")
    if (order == 2 and not rnnlm) or opts.decode_type == "Greedy":
        return test_ctc.make_decoder(opts, index2word)
    from ctc_pytorch_amd.utils.ctcDecoder import BeamDecoder
    return BeamDecoder(index2word, beam_width=opts.beam_width, blank_index=0, space_idx=-1, lm_path=opts.lm_path, lm_alpha=opts.lm_alpha,
                       lm_order=order, **rnnlm)


def apply_argv(conf, a):
    """The command line's switches laid over the YAML's keys; a switch that was not given leaves its key alone."""
    if a.error_report:
        conf["error_report"] = True
    if a.score_map is not None:
        conf["score_map"] = a.score_map
    if a.score_map_cols is not None:
        conf["score_map_cols"] = a.score_map_cols
    if a.mask_padding:
        conf["mask_padding"] = True
    if a.ctm is not None:
        conf["ctm"] = a.ctm
    if a.ctm_frame_shift is not None:
        conf["ctm_frame_shift"] = a.ctm_frame_shift
    if a.device_context:
        conf["device_context"] = True
    if a.lm_order is not None:
        conf["lm_order"] = a.lm_order
    for key in ("rnnlm_path", "rnnlm_weight", "rnnlm_nbest", "rnnlm_len_bonus"):
        if getattr(a, key) is not None:
            conf[key] = getattr(a, key)
    return conf


def arg_parser():
    ap = argparse.ArgumentParser(description="decode + score a ctc_best_model.pkl on MI355X, optionally with the utterance lengths passed to the model")
    ap.add_argument("--conf", help="conf file (same keys as timit/conf/ctc_config.yaml, plus mask_padding)")
    ap.add_argument("--mask-padding", action="store_true", help="tell the model every utterance's real frames (default: the YAML's mask_padding, else off)")
    ap.add_argument("--error-report", action="store_true", help="log the error breakdown (sub / del / ins, top confusions) after the CER / WER lines (default: the YAML's error_report, else off)")
    ap.add_argument("--score-map", default=None, help="three-column phone table the breakdown is scored under (default: the YAML's score_map, else none)")
    ap.add_argument("--score-map-cols", default=None, choices=["60-48", "60-39", "48-39"], help="which fold of the table (default: the YAML's score_map_cols, else 48-39)")
    ap.add_argument("--ctm", default=None, metavar="PATH", help="write the recognised tokens with start, duration and confidence to this NIST CTM file (default: the YAML's ctm, else off)")
    ap.add_argument("--ctm-frame-shift", default=None, type=float, help="seconds per model input frame (default: the YAML's ctm_frame_shift, else 0.01)")
    ap.add_argument("--device-context", action="store_true", help="read the archive as base features and splice / skip / pad on the GPU (default: the YAML's device_context, else off)")
    ap.add_argument("--lm-order", default=None, type=int, choices=[2, 3], help="order of the beam search's LM: 3 reads the ARPA file's 3-gram section (default: the YAML's lm_order, else 2)")
    ap.add_argument("--rnnlm-path", default=None, metavar="PATH", help="rescore the beam search's n-best list with this RNN LM package (default: the YAML's rnnlm_path, else off)")
    ap.add_argument("--rnnlm-weight", default=None, type=float, help="weight of the LM's log-probability (default: the YAML's rnnlm_weight, else 0.5)")
    ap.add_argument("--rnnlm-nbest", default=None, type=int, help="labellings per utterance handed to the LM, at most the beam width (default: the YAML's rnnlm_nbest, else 10)")
    ap.add_argument("--rnnlm-len-bonus", default=None, type=float, help="added per label of a labelling (default: the YAML's rnnlm_len_bonus, else 0)")
    return ap


def main(conf, test_loader=None, index2word=None, log=print):
    """steps/test_ctc.main for the same YAML plus `mask_padding`.  Returns (CER, WER)."""
    from ctc_pytorch_amd import parallel
    from ctc_pytorch_amd.steps.train_ctc import Config
    opts = Config()
    for k, v in conf.items():
        setattr(opts, k, v)
    report = bool(getattr(opts, "error_report", False))
    ctm = ctm_options(opts)
    context = device_context(opts)
    if not epoch_options(opts) and not report and not ctm and context is None and lm_order_option(opts) == 2 and not rnnlm_options(opts):
        return test_ctc.main(conf, test_loader=test_loader, index2word=index2word, log=log)
    if not getattr(opts, "use_gpu", True):
        raise RuntimeError("ctc_pytorch_amd: use_gpu must be True -- the HIP path has no CPU fallback")
    rank, world, local = parallel.init_from_env()
    device = torch.device("cuda", local)
    model, _ = test_ctc.load_package(os.path.join(opts.checkpoint_dir, opts.exp_name, "ctc_best_model.pkl"), device)
    if test_loader is None:
        from ctc_pytorch_amd.utils.data_loader import SpeechDataLoader, SpeechDataset, Vocab
        vocab = Vocab(opts.vocab_file)
        index2word = vocab.index2word
        if context is None:
            test_loader = SpeechDataLoader(SpeechDataset(vocab, opts.test_scp_path, opts.test_lab_path, opts), batch_size=opts.batch_size,
                                           shuffle=False, num_workers=opts.num_workers)
        else:
            from ctc_pytorch_amd.utils.data_loader import BaseFeatureLoader
            test_loader = BaseFeatureLoader(SpeechDataset(vocab, opts.test_scp_path, opts.test_lab_path, opts, base_features=True),
                                            batch_size=opts.batch_size, shuffle=False, num_workers=opts.num_workers)
    if context is not None:                                # (a loader handed in must be a base-feature loader too)
        from ctc_pytorch_amd.utils.data_loader import DeviceContext
        test_loader = _labels_on_host(DeviceContext(test_loader, device, context))
    decoder = make_decoder(opts, index2word)
    stats = class_map = None
    if report:
        from ctc_pytorch_amd.utils.scoring import ErrorStats
        stats = ErrorStats(index2word)
        class_map = report_options(opts, index2word).get("score_map")
    start = time.time()
    cer, wer = decode_and_score(model, test_loader, decoder, index2word, device, verbose=bool(getattr(opts, "verbose", False)), log=log,
                                mask_padding=bool(epoch_options(opts)), rank=rank, world=world, stats=stats, class_map=class_map,
                                n_skip_frame=getattr(opts, "n_skip_frame", 1), **ctm)
    if rank == 0:
        log("time used for decode: %.4f minutes." % ((time.time() - start) / 60.0))
    return cer, wer


if __name__ == "__main__":
    import yaml
    a = arg_parser().parse_args()
    main(apply_argv(yaml.safe_load(open(a.conf, "r")), a))
