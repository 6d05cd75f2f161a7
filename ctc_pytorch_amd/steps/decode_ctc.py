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
from ctc_pytorch_amd.steps.train_ctc import epoch_options, input_frames_from_fraction, report_options  # noqa: E402


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


def decode_and_score(model, loader, decoder, index2word, device, verbose=False, log=print, mask_padding=True, rank=0, world=1,
                     stats=None, class_map=None):
    """steps/test_ctc.decode_and_score_sharded (one process: decode_and_score) over the length-aware pair; mask_padding=False: over the
    plain one.  stats (a host utils.scoring.ErrorStats): the loop scores through _ScoringDecoder, the stats are summed over the ranks
    beside the four totals, and rank 0 logs the report after the CER / WER lines."""
    if mask_padding:
        model, loader = length_aware(model, loader)
    if stats is None:
        return test_ctc.decode_and_score_sharded(model, loader, decoder, index2word, device, rank, world, verbose=verbose, log=log)
    out = test_ctc.decode_and_score_sharded(model, loader, _ScoringDecoder(decoder, stats, index2word, class_map), index2word, device, rank,
                                            world, verbose=verbose, log=log)
    if world > 1:
        import torch.distributed as dist
        t = stats.state().to(device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        stats._state.copy_(t)
    if rank == 0:
        log(stats.report())
    return out


def main(conf, test_loader=None, index2word=None, log=print):
    """steps/test_ctc.main for the same YAML plus `mask_padding`.  Returns (CER, WER)."""
    from ctc_pytorch_amd import parallel
    from ctc_pytorch_amd.steps.train_ctc import Config
    opts = Config()
    for k, v in conf.items():
        setattr(opts, k, v)
    report = bool(getattr(opts, "error_report", False))
    if not epoch_options(opts) and not report:
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
        test_loader = SpeechDataLoader(SpeechDataset(vocab, opts.test_scp_path, opts.test_lab_path, opts), batch_size=opts.batch_size,
                                       shuffle=False, num_workers=opts.num_workers)
    decoder = test_ctc.make_decoder(opts, index2word)
    stats = class_map = None
    if report:
        from ctc_pytorch_amd.utils.scoring import ErrorStats
        stats = ErrorStats(index2word)
        class_map = report_options(opts, index2word).get("score_map")
    start = time.time()
    cer, wer = decode_and_score(model, test_loader, decoder, index2word, device, verbose=bool(getattr(opts, "verbose", False)), log=log,
                                mask_padding=bool(epoch_options(opts)), rank=rank, world=world, stats=stats, class_map=class_map)
    if rank == 0:
        log("time used for decode: %.4f minutes." % ((time.time() - start) / 60.0))
    return cer, wer


if __name__ == "__main__":
    import yaml
    ap = argparse.ArgumentParser(description="decode + score a ctc_best_model.pkl on MI355X, optionally with the utterance lengths passed to the model")
    ap.add_argument("--conf", help="conf file (same keys as timit/conf/ctc_config.yaml, plus mask_padding)")
    ap.add_argument("--mask-padding", action="store_true", help="tell the model every utterance's real frames (default: the YAML's mask_padding, else off)")
    ap.add_argument("--error-report", action="store_true", help="log the error breakdown (sub / del / ins, top confusions) after the CER / WER lines (default: the YAML's error_report, else off)")
    ap.add_argument("--score-map", default=None, help="three-column phone table the breakdown is scored under (default: the YAML's score_map, else none)")
    ap.add_argument("--score-map-cols", default=None, choices=["60-48", "60-39", "48-39"], help="which fold of the table (default: the YAML's score_map_cols, else 48-39)")
    a = ap.parse_args()
    conf = yaml.safe_load(open(a.conf, "r"))
    if a.error_report:
        conf["error_report"] = True
    if a.score_map is not None:
        conf["score_map"] = a.score_map
    if a.score_map_cols is not None:
        conf["score_map_cols"] = a.score_map_cols
    if a.mask_padding:
        conf["mask_padding"] = True
    main(conf)
