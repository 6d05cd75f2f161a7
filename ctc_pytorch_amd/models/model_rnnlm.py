"""RNN language model over the acoustic model's label inventory, on the gfx950 HIP kernels (the reference's to-do list names "Combine with
RNN-LM" and "Beam search with RNN-LM"; it has neither).

The model is the acoustic model's recurrent stack fed by an embedding: embed (nn.Embedding) -> rnns.{l} (models.model_ctc.BatchRNN,
unidirectional, no BatchNorm on layer 0) -> fc (BatchNorm1d + bias-free Linear, or the Linear alone) -> logits.  Lengths are always passed
down, so padding reaches no BatchNorm statistic.

The vocabulary is the acoustic model's, id for id.  Class 0 -- the CTC blank -- never occurs in a labelling, so it serves as the ONE
sentence-boundary symbol: a labelling y_1 .. y_l is the input [0, y_1 .. y_l] with the target [y_1 .. y_l, 0], l + 1 steps, and
ln P(y, boundary) is the sum of the l + 1 token log-probs.  Positions behind a sequence carry input 0 and target IGNORE.
"""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from ctc_pytorch_amd import nn, ops  # noqa: E402
from ctc_pytorch_amd.models.model_ctc import BatchRNN, _native_rnn  # noqa: E402

BOUNDARY = 0          # the CTC blank: sentence start on the input side, sentence end on the target side
IGNORE = -100         # target of a position behind its sequence

_RNN_NAMES = {"LSTM": nn.LSTM, "GRU": nn.GRU, "RNN": nn.RNN}


def lm_batch(labellings, boundary=BOUNDARY, ignore_index=IGNORE):
    """Host half of a batch: a list of label-id sequences -> (ids (L+1, B), targets (L+1, B), lens (B)) int64 numpy arrays, time-major, L the
    longest labelling; what ctcn_lm_pack_nbest builds on the device from an n-best list.  An empty labelling is the one-step sequence
    boundary -> boundary."""
    rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in labellings]
    if not rows:
        raise ValueError("lm_batch: no labellings")
    B, L = len(rows), max(len(r) for r in rows)
    ids = np.zeros((L + 1, B), dtype=np.int64)
    tgt = np.full((L + 1, B), ignore_index, dtype=np.int64)
    lens = np.zeros(B, dtype=np.int64)
    ids[0, :] = boundary
    for b, r in enumerate(rows):
        n = len(r)
        ids[1:n + 1, b] = r
        tgt[:n, b] = r
        tgt[n, b] = boundary
        lens[b] = n + 1
    return ids, tgt, lens


def length_sorted_batches(labellings, batch_size, shuffle_seed=None):
    """Minibatches of sentence indices: sentences sorted by length (stable), cut into runs of batch_size, the ORDER OF THE RUNS shuffled by
    shuffle_seed (None: left in length order).  Every sentence appears once; a batch pads to its own longest sentence only."""
    order = sorted(range(len(labellings)), key=lambda i: len(labellings[i]))
    batches = [order[i:i + int(batch_size)] for i in range(0, len(order), int(batch_size))]
    if shuffle_seed is not None:
        perm = np.random.RandomState(int(shuffle_seed)).permutation(len(batches))
        batches = [batches[i] for i in perm]
    return batches


class RNNLM(nn.Module):
    def __init__(self, num_class, emb_size=128, hidden_size=256, layers=2, rnn_type=nn.LSTM, batch_norm=True, drop_out=0.1):
        super().__init__()
        if isinstance(rnn_type, str):
            rnn_type = _RNN_NAMES[rnn_type.split(".")[-1].upper()]
        rnn_type = _native_rnn(rnn_type)
        if int(num_class) < 2 or int(layers) < 1:
            raise ValueError("RNNLM: num_class >= 2 and layers >= 1")
        self.num_class, self.emb_size, self.hidden_size, self.layers = int(num_class), int(emb_size), int(hidden_size), int(layers)
        self.rnn_type, self.batch_norm, self.drop_out = rnn_type, bool(batch_norm), float(drop_out)
        self.embed = nn.Embedding(self.num_class, self.emb_size)
        blocks = [BatchRNN(input_size=self.emb_size if n == 0 else self.hidden_size, hidden_size=self.hidden_size, rnn_type=rnn_type,
                           bidirectional=False, batch_norm=bool(n) and self.batch_norm, dropout=self.drop_out) for n in range(self.layers)]
        self.rnns = nn.Sequential(*blocks)
        head = nn.Linear(self.hidden_size, self.num_class, bias=False)
        self.fc = nn.Sequential(nn.BatchNorm1d(self.hidden_size), head) if self.batch_norm else head

    def forward(self, ids_tb, lengths):
        """ids_tb (T, B) integer ids (host or device), lengths (B) steps per sequence (>= 1) -> logits (T, B, V) float32; positions behind a
        sequence give logits 0."""
        dev = self.embed.weight.device
        if dev.type != "cuda":
            raise RuntimeError("ctc_pytorch_amd: RNNLM on %s -- the HIP path needs a ROCm device (there is no CPU fallback)" % dev)
        ids = ops.token_ids(ids_tb, self.num_class, dev, "RNNLM ids")
        if ids.dim() != 2:
            raise ValueError("RNNLM: ids must be (T, B)")
        T, B = ids.shape
        lens = ops.frame_lengths(lengths, dev, batch=B, tmax=T)
        h = self.embed(ids)
        for block in self.rnns:
            h = block(h, lengths=lens)
        h = h.reshape(T * B, -1)
        if isinstance(self.fc, nn.Sequential):
            z = self.fc[1](self.fc[0](h, lengths=lens))
        else:
            z = self.fc(ops.mask_frames(h.view(T, B, -1), lens, "tbc").view(T * B, -1))
        return z.view(T, B, self.num_class)

    @staticmethod
    def _rows(labels, label_lengths):
        lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else labels
        if label_lengths is None:
            return [np.asarray(r, dtype=np.int64) for r in lab]
        n = label_lengths.detach().cpu().numpy() if torch.is_tensor(label_lengths) else np.asarray(label_lengths)
        return [np.asarray(lab[b][: int(n[b])], dtype=np.int64) for b in range(len(n))]

    def loss(self, labels, label_lengths=None, reduction="mean"):
        """Cross-entropy of a batch of labellings (padded (B, Lmax) ids with label_lengths, or a list of id sequences), every sequence with
        its boundary step: 'mean' is per token (boundary steps included), 'sum' the batch total, 'none' the (L+1, B) token losses."""
        ids, tgt, lens = lm_batch(self._rows(labels, label_lengths))
        logits = self.forward(ids, lens)
        return ops.cross_entropy(logits, tgt, IGNORE, reduction)

    def score_packed(self, in_ids, targets, lens):
        """ln P of every sequence of a packed device batch (ops.pack_nbest): (S) float64 on the device.  Evaluation mode, no gradient, no
        host synchronisation."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                return ops.sequence_log_prob(self.forward(in_ids, lens), targets, IGNORE)
        finally:
            self.train(was_training)

    def score(self, labellings):
        """ln P(y, boundary) of every labelling of a list of id sequences: (B) float64 on the device."""
        ids, tgt, lens = lm_batch(labellings)
        dev = self.embed.weight.device
        return self.score_packed(ids, torch.from_numpy(tgt).to(dev), lens)

    @staticmethod
    def save_package(model, optimizer=None, epoch=None, loss_results=None, dev_loss_results=None):
        """Checkpoint dict in the style of CTC_Model.save_package: the constructor arguments, the state_dict and what the driver adds."""
        name = [k for k, v in _RNN_NAMES.items() if v is model.rnn_type]
        package = {"num_class": model.num_class, "emb_size": model.emb_size, "hidden_size": model.hidden_size, "layers": model.layers,
                   "rnn_type": name[0] if name else model.rnn_type, "batch_norm": model.batch_norm, "_drop_out": model.drop_out,
                   "state_dict": model.state_dict()}
        optional = {"optim_dict": None if optimizer is None else optimizer.state_dict(), "epoch": epoch}
        package.update({k: v for k, v in optional.items() if v is not None})
        if loss_results is not None:
            package.update(loss_results=loss_results, dev_loss_results=dev_loss_results)
        return package

    @staticmethod
    def load_package(package, device=None):
        """An RNNLM from a package (the dict, or the path of a file torch.save wrote it to), moved to `device` if one is given."""
        if not isinstance(package, dict):
            package = torch.load(package, map_location="cpu", weights_only=False)
        model = RNNLM(package["num_class"], emb_size=package["emb_size"], hidden_size=package["hidden_size"], layers=package["layers"],
                      rnn_type=package["rnn_type"], batch_norm=package["batch_norm"], drop_out=package["_drop_out"])
        model.load_state_dict(package["state_dict"])
        return model if device is None else model.to(device)
