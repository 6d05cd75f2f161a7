"""Train an RNN language model (models/model_rnnlm.RNNLM) on the recipe's label transcripts.

    python -m ctc_pytorch_amd.steps.train_rnnlm --conf conf/rnnlm.yaml [--epochs N] [--output PATH] ...

YAML keys (every one has a command-line switch that overrides it):
  vocab_file                      the `units` file of the acoustic recipe (utils/data_loader.Vocab: ids 0 / 1 are blank / UNK)
  train_lab_path, valid_lab_path  the label files the acoustic driver reads: one `utt symbol symbol ...` line per utterance
  emb_size 128, hidden_size 256, layers 2, rnn_type "LSTM", batch_norm true, drop_out 0.1
  batch_size 32, num_epoches 20, init_lr 1e-3, lr_decay 0.5, weight_decay 0.0, max_grad_norm (absent: no clipping), seed 1234
  output                          where the best package goes (absent: nothing is written)

Sentences are sorted by length and cut into minibatches (the order of the minibatches is reshuffled every epoch); FlatAdam steps on the
mean token cross-entropy; the dev perplexity is logged every epoch; the learning rate is multiplied by lr_decay whenever the dev loss
has not fallen (the rule of steps/train_ctc.py, without its ten-epoch patience: an LM epoch is seconds); the package of the best dev loss is
kept and written.
"""
import argparse
import copy
import json
import math
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from ctc_pytorch_amd.models.model_rnnlm import RNNLM, length_sorted_batches  # noqa: E402
from ctc_pytorch_amd.optim import FlatAdam  # noqa: E402

DEFAULTS = {"emb_size": 128, "hidden_size": 256, "layers": 2, "rnn_type": "LSTM", "batch_norm": True, "drop_out": 0.1, "batch_size": 32,
            "num_epoches": 20, "init_lr": 1e-3, "lr_decay": 0.5, "weight_decay": 0.0, "max_grad_norm": None, "seed": 1234, "output": None}


def read_labels(lab_path, vocab):
    """The label file of the acoustic recipe as a list of id lists (unknown symbols become UNK, as in SpeechDataset); empty lines are dropped."""
    unk = vocab.word2index["UNK"]
    rows = []
    with open(lab_path, "r") as fh:
        for line in fh:
            fields = line.strip().split(" ", 1)
            if len(fields) == 2 and fields[1].strip():
                rows.append([vocab.word2index.get(c, unk) for c in fields[1].split()])
    return rows


def arg_parser():
    ap = argparse.ArgumentParser(description="train an RNN language model on label transcripts, on MI355X")
    ap.add_argument("--conf", default=None, help="YAML file with the keys of the module docstring")
    ap.add_argument("--vocab-file", default=None)
    ap.add_argument("--train-lab-path", default=None)
    ap.add_argument("--valid-lab-path", default=None)
    ap.add_argument("--emb-size", type=int, default=None)
    ap.add_argument("--hidden-size", type=int, default=None)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--rnn-type", default=None, choices=["LSTM", "GRU", "RNN"])
    ap.add_argument("--no-batch-norm", action="store_true")
    ap.add_argument("--drop-out", type=float, default=None)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--epochs", type=int, default=None, dest="num_epoches")
    ap.add_argument("--init-lr", type=float, default=None)
    ap.add_argument("--lr-decay", type=float, default=None)
    ap.add_argument("--weight-decay", type=float, default=None)
    ap.add_argument("--max-grad-norm", type=float, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--output", default=None, help="file the best package is written to")
    return ap


def apply_argv(conf, a):
    """The command line's switches laid over the YAML's keys; a switch that was not given leaves its key alone."""
    conf = dict(conf or {})
    for key in ("vocab_file", "train_lab_path", "valid_lab_path", "emb_size", "hidden_size", "layers", "rnn_type", "drop_out", "batch_size",
                "num_epoches", "init_lr", "lr_decay", "weight_decay", "max_grad_norm", "seed", "output"):
        value = getattr(a, key)
        if value is not None:
            conf[key] = value
    if a.no_batch_norm:
        conf["batch_norm"] = False
    return conf


def options(conf):
    """DEFAULTS overlaid with `conf`; an unknown key is an error (a misspelt key would otherwise train with the default in silence)."""
    known = set(DEFAULTS) | {"vocab_file", "train_lab_path", "valid_lab_path"}
    unknown = sorted(set(conf) - known)
    if unknown:
        raise ValueError("train_rnnlm: unknown keys %s" % unknown)
    opts = dict(DEFAULTS)
    opts.update(conf)
    if opts["max_grad_norm"] is not None and not float(opts["max_grad_norm"]) > 0:
        raise ValueError("train_rnnlm: max_grad_norm must be positive")
    if not 0.0 < float(opts["lr_decay"]) <= 1.0:
        raise ValueError("train_rnnlm: lr_decay must lie in (0, 1]")
    return opts


def evaluate(model, sentences, batch_size):
    """(cross-entropy per token in nats, tokens) of `sentences` in evaluation mode; every sentence counts its boundary step."""
    was_training = model.training
    model.eval()
    total = None
    try:
        with torch.no_grad():
            for batch in length_sorted_batches(sentences, batch_size):
                part = model.loss([sentences[i] for i in batch], reduction="sum").double()
                total = part if total is None else total + part
    finally:
        model.train(was_training)
    tokens = sum(len(s) + 1 for s in sentences)
    return float(total) / max(tokens, 1), tokens


def main(conf, train_sentences=None, dev_sentences=None, num_class=None, log=print):
    """Train; returns (model, dict(loss=[...], dev_loss=[...], best_dev_loss=...)).  train_sentences / dev_sentences (lists of id lists) and
    num_class may be handed in instead of the three file keys."""
    opts = options(conf)
    if train_sentences is None:
        from ctc_pytorch_amd.utils.data_loader import Vocab
        vocab = Vocab(opts["vocab_file"])
        num_class = vocab.n_words
        train_sentences = read_labels(opts["train_lab_path"], vocab)
        dev_sentences = read_labels(opts["valid_lab_path"], vocab)
    if not train_sentences or not dev_sentences or num_class is None:
        raise ValueError("train_rnnlm: needs training sentences, dev sentences and num_class")
    device = torch.device("cuda", 0)
    torch.manual_seed(int(opts["seed"]))
    np.random.seed(int(opts["seed"]))
    model = RNNLM(num_class, emb_size=opts["emb_size"], hidden_size=opts["hidden_size"], layers=opts["layers"], rnn_type=opts["rnn_type"],
                  batch_norm=opts["batch_norm"], drop_out=opts["drop_out"]).to(device)
    log("Number of parameters %d" % sum(p.numel() for p in model.parameters()))
    clip = {} if opts["max_grad_norm"] is None else {"max_grad_norm": float(opts["max_grad_norm"])}
    optimizer = FlatAdam(model, lr=float(opts["init_lr"]), weight_decay=float(opts["weight_decay"]), **clip)
    loss_results, dev_loss_results = [], []
    best, best_state = float("inf"), None
    for epoch in range(1, int(opts["num_epoches"]) + 1):
        model.train()
        batches = length_sorted_batches(train_sentences, opts["batch_size"], shuffle_seed=int(opts["seed"]) + epoch)
        running = None
        for batch in batches:
            loss = model.loss([train_sentences[i] for i in batch], reduction="mean")
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            running = loss.detach() if running is None else running + loss.detach()
        train_loss = float(running) / len(batches)          # (the one read of the epoch)
        dev_loss, tokens = evaluate(model, dev_sentences, opts["batch_size"])
        loss_results.append(train_loss)
        dev_loss_results.append(dev_loss)
        log("Epoch %d done, learning_rate: %.6f, train_loss: %.4f, dev_loss: %.4f, dev_ppl: %.3f (%d tokens)"
            % (epoch, optimizer.param_groups[0]["lr"], train_loss, dev_loss, math.exp(min(dev_loss, 700.0)), tokens))
        if dev_loss < best:
            best = dev_loss
            best_state = (copy.deepcopy(model.state_dict()), copy.deepcopy(optimizer.state_dict()))
        else:                                               # the dev loss stopped falling: back to the best state, smaller steps
            lr = optimizer.param_groups[0]["lr"] * float(opts["lr_decay"])
            model.load_state_dict(best_state[0])
            optimizer.load_state_dict(best_state[1])        # (brings the best epoch's learning rate along: set the decayed one after it)
            optimizer.param_groups[0]["lr"] = lr
        log(json.dumps(dict(epoch=epoch, train_loss=train_loss, dev_loss=dev_loss, dev_ppl=math.exp(min(dev_loss, 700.0)))))
    if best_state is not None:
        model.load_state_dict(best_state[0])
    if opts["output"]:
        out_dir = os.path.dirname(os.path.abspath(opts["output"]))
        os.makedirs(out_dir, exist_ok=True)
        torch.save(RNNLM.save_package(model, epoch=len(loss_results), loss_results=loss_results, dev_loss_results=dev_loss_results), opts["output"])
    return model, dict(loss=loss_results, dev_loss=dev_loss_results, best_dev_loss=best)


if __name__ == "__main__":
    import yaml
    a = arg_parser().parse_args()
    main(apply_argv(yaml.safe_load(open(a.conf, "r")) if a.conf else {}, a))
