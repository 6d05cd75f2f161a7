"""HIP-backed drop-ins for the `torch.nn` names the reference drivers use.

The reference's train/test scripts do `import torch.nn as nn` and then `from models.model_ctc import *`
(timit/steps/train_ctc.py:13,16; test_ctc.py:9,13), so whatever `nn` our models.model_ctc exports shadows
theirs: `nn.CTCLoss(reduction='sum')` (train_ctc.py:144) and `supported_rnn = {'nn.LSTM': nn.LSTM, ...}`
(:20) resolve to the classes below with the drivers textually unchanged.  Each class subclasses the torch
module purely as a *parameter container* (same constructor, same init => same-seed equality, identical
state_dict keys) and replaces `forward` with calls into libctcn.so.  Names not defined here fall through to
torch.nn (module-level __getattr__).
"""
import torch
import torch.nn as _tnn

from . import ops
from .optim import ALIGN

Module = _tnn.Module
Sequential = _tnn.Sequential
Parameter = _tnn.Parameter


def __getattr__(name):          # everything else (init, functional, ...) is plain torch.nn
    return getattr(_tnn, name)


def _flat_grad_of(params):
    """The flat gradient buffer of optim.FlatAdam if `params` are all homed in it and together cover it exactly once, else None.  Between two
    views there may lie optim.flat_layout's alignment padding (fewer than optim.ALIGN elements, which hold zero and add nothing to a norm)."""
    grads = [getattr(p, "_ctcn_grad", None) for p in params]
    if not grads or any(g is None for g in grads):
        return None
    flat = grads[0]._base
    if flat is None or flat.dim() != 1 or not flat.is_contiguous():
        return None
    spans = sorted({(g.data_ptr(), g.numel()) for g in grads if g._base is not None and g._base.data_ptr() == flat.data_ptr()
                    and g._base.numel() == flat.numel() and g.is_contiguous()})
    if len(spans) != len({id(g) for g in grads}):
        return None
    cur = flat.data_ptr()
    for ptr, n in spans:
        if not 0 <= ptr - cur < 4 * ALIGN:
            return None
        cur = ptr + 4 * n
    return flat if cur == flat.data_ptr() + 4 * flat.numel() else None


def _clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ (the reference carries it at train_ctc.py:64).  When every parameter lives in one optim.FlatAdam and
    together they cover its flat gradient buffer, the norm and the in-place scaling run on that buffer with the library's kernels
    (ops.clip_grad_norm_: same semantics, deterministic norm) after the weight-gradient side stream has been joined -- torch's own
    kernels on the 25 p.grad views would race with gradients still in flight there.  Any other parameter list is torch's business (the
    side stream is still joined first if a parameter is FlatAdam-homed)."""
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    flat = _flat_grad_of(params) if float(norm_type) in (2.0, float("inf")) else None
    if any(getattr(p, "_ctcn_grad", None) is not None for p in params):
        ops.join_side_stream()
    if flat is None:
        return _tnn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    return ops.clip_grad_norm_(flat, max_norm, norm_type, error_if_nonfinite)


def _make_utils():
    """`nn.utils`: torch.nn.utils with clip_grad_norm_ replaced; every other name (rnn, parameters_to_vector, ...) resolves to torch's."""
    import sys
    import types
    m = types.ModuleType(__name__ + ".utils", _make_utils.__doc__)
    m.clip_grad_norm_ = _clip_grad_norm_
    m.__getattr__ = lambda name: getattr(_tnn.utils, name)
    sys.modules[m.__name__] = m
    return m


utils = _make_utils()


class _RecurrentMixin:
    _cell = None

    def _check(self):
        if self.num_layers != 1 or self.bias or self.batch_first or getattr(self, "proj_size", 0):
            raise NotImplementedError(
                "ctc_pytorch_amd.nn.%s supports what the reference constructs: num_layers=1, bias=False, "
                "batch_first=False (model_ctc.py:24-25)" % type(self).__name__)
        if float(self.dropout) != 0.0:
            raise NotImplementedError("inter-layer dropout of a 1-layer RNN is a no-op; got dropout=%r" % self.dropout)

    def forward(self, x, hx=None, drop_p=0.0):
        """drop_p: the dropout that FOLLOWS this layer (BatchRNN), applied to the returned output in training mode -- inside the
        recurrent kernel where that is possible (ops.rnn_layer), as a dropout pass otherwise; the same values either way."""
        if hx is not None:
            raise NotImplementedError("initial state is always zero on the reference path (model_ctc.py:33)")
        self._check()
        w1 = (self.weight_ih_l0_reverse, self.weight_hh_l0_reverse) if self.bidirectional else (None, None)
        H = self.hidden_size
        if H % 4 == 0:
            y = ops.rnn_layer(x, self.weight_ih_l0, self.weight_hh_l0, w1[0], w1[1], self._cell, self.training, drop_p if self.training else 0.0)
            return y, None
        # The kernels move rows of W_hh / h in 16-byte pieces (H % 4 == 0).  Any other hidden size (nn.LSTM takes every H,
        # model_ctc.py:24-25) runs as the next multiple of 4 with all-zero weights for the extra units: their pre-activations are 0,
        # so c = h = 0 for every cell type at every step and the real units never see them; the padding / slicing around the
        # kernels is plain tensor plumbing (autograd routes the gradients of the real rows back through it).
        Hp, G = H + (4 - H % 4), {"lstm": 4, "gru": 3, "tanh": 1}[self._cell]

        def pad(w_ih, w_hh):
            wi = _tnn.functional.pad(w_ih.view(G, H, -1), (0, 0, 0, Hp - H)).reshape(G * Hp, -1)
            wh = _tnn.functional.pad(w_hh.view(G, H, H), (0, Hp - H, 0, Hp - H)).reshape(G * Hp, Hp)
            return wi.contiguous(), wh.contiguous()

        p0 = pad(self.weight_ih_l0, self.weight_hh_l0)
        p1 = pad(*w1) if self.bidirectional else (None, None)
        yp = ops.rnn_layer(x, p0[0], p0[1], p1[0], p1[1], self._cell, self.training)
        T, B, _ = yp.shape
        D = 2 if self.bidirectional else 1
        y = ops.contiguous(yp.view(T, B, D, Hp)[..., :H]).view(T, B, D * H)               # drop the padded units (strided gather kernel)
        return ops.dropout(y, drop_p, self.training), None

    def flatten_parameters(self):
        return None


class LSTM(_RecurrentMixin, _tnn.LSTM):
    """nn.LSTM(input_size, hidden_size, bidirectional=..., bias=False): gate rows i,f,g,o."""
    _cell = "lstm"


class GRU(_RecurrentMixin, _tnn.GRU):
    """nn.GRU(..., bias=False): gate rows r,z,n."""
    _cell = "gru"


class RNN(_RecurrentMixin, _tnn.RNN):
    """nn.RNN(..., bias=False), tanh."""
    _cell = "tanh"

    def _check(self):
        super()._check()
        if self.nonlinearity != "tanh":
            raise NotImplementedError("only nonlinearity='tanh' (the nn.RNN default the reference uses)")


class BatchNorm1d(_tnn.BatchNorm1d):
    """(N,C) or (N,C,L) input, statistics per channel over N*L -- BatchRNN feeds (T,C,B) views (model_ctc.py:29-32)."""

    fuse_relu = False

    def forward(self, x, lengths=None):
        """lengths (frames per utterance; None: every row counts): statistics over the real frames only and zeros at the padded ones
        (ops.batch_norm_masked).  (N,C) rows are time-major, N = T * len(lengths); (N,C,L) as fed by BatchRNN is (T,C,B); a contiguous
        (N,C,L) tensor is (B,C,T)."""
        if not (self.affine and self.track_running_stats):
            raise NotImplementedError("affine=True, track_running_stats=True only (nn.BatchNorm1d defaults)")
        C = self.num_features
        training = self.training
        mom = 0.1 if self.momentum is None else self.momentum
        nbt = self.num_batches_tracked              # (+= 1 by the statistics kernel in training: no launch of its own)
        if x.dim() == 2:
            return ops.batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, x.shape[0], C, 1, training,
                                  mom, self.eps, self.fuse_relu, nbt, lengths=lengths)
        if x.dim() != 3 or x.shape[1] != C:
            raise ValueError("BatchNorm1d expects (N,C) or (N,C,L)")
        xt = x.transpose(1, 2)                     # (N,L,C)
        if xt.is_contiguous():                     # the reference's x.transpose(-1,-2) of a (T,B,C) tensor
            N, Lq = xt.shape[0], xt.shape[1]
            y = ops.batch_norm(xt, self.weight, self.bias, self.running_mean, self.running_var, N * Lq, C, 1, training, mom,
                               self.eps, self.fuse_relu, nbt, lengths=lengths)
            return y.view(N, Lq, C).transpose(1, 2)
        x = ops.contiguous(x)
        return ops.batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, x.shape[0], C, x.shape[2], training,
                              mom, self.eps, self.fuse_relu, nbt, lengths=lengths, frame=None if lengths is None else 1)


class BatchNorm2d(_tnn.BatchNorm2d):
    """NCHW, statistics per channel over (B,T,F) (model_ctc.py:47,63)."""

    fuse_relu = False

    def forward(self, x, drop_p=0.0, lengths=None):
        """drop_p > 0 (LayerCNN, training): the layer's dropout rides along with the apply pass (ops.batch_norm).
        lengths (frames per image on axis 2; None: every element counts): statistics over the real frames, zeros at the padded ones."""
        if not (self.affine and self.track_running_stats):
            raise NotImplementedError("affine=True, track_running_stats=True only")
        if x.dim() != 4 or x.shape[1] != self.num_features:
            raise ValueError("BatchNorm2d expects (B,C,H,W)")
        mom = 0.1 if self.momentum is None else self.momentum
        x = ops.contiguous(x)
        return ops.batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, x.shape[0], x.shape[1],
                              x.shape[2] * x.shape[3], self.training, mom, self.eps, self.fuse_relu, self.num_batches_tracked,
                              drop_p=float(drop_p) if self.training else 0.0, lengths=lengths, frame=None if lengths is None else x.shape[3])


class Linear(_tnn.Linear):
    def forward(self, x):
        if self.bias is not None:
            raise NotImplementedError("bias=False only (model_ctc.py:137,139)")
        shp = x.shape
        y = ops.linear(x.reshape(-1, shp[-1]), self.weight)
        return y.view(*shp[:-1], self.out_features)


class Conv2d(_tnn.Conv2d):
    def forward(self, x):
        if self.groups != 1 or tuple(self.dilation) != (1, 1) or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise NotImplementedError("plain Conv2d (groups=1, dilation=1, zero padding) only (model_ctc.py:46)")
        return ops.conv2d(x, self.weight, self.bias, self.stride, self.padding)


class ReLU(_tnn.Module):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def forward(self, x):
        return ops.relu(x)


class Dropout(_tnn.Dropout):
    def forward(self, x):
        return ops.dropout(x, self.p, self.training)


class LogSoftmax(_tnn.Module):
    def __init__(self, dim=None):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        if self.dim not in (-1, x.dim() - 1):
            raise NotImplementedError("LogSoftmax over the last dim only (model_ctc.py:140)")
        return ops.log_softmax(x)


class CTCLoss(_tnn.Module):
    """nn.CTCLoss(blank=0, reduction='mean', zero_infinity=False) with torch's whole contract: any blank in [0, C), reduction 'none' /
    'sum' / 'mean' (each loss divided by its target length clamped to >= 1, then averaged over the batch), zero_infinity, padded (B, S) or
    concatenated 1-D targets, lengths as tensors (host or device), lists or tuples, unbatched (T, C) input.  The reference calls it with
    reduction='sum' (train_ctc.py:144,47).  float32 log-probs on the device only.

    Under data parallelism 'mean' averages over the rank's OWN shard: the drivers (steps/train_ctc.main, bench.py) keep 'sum' / B_global,
    which is what the reference's single-process mean of the global batch amounts to."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in ("none", "sum", "mean"):
            raise ValueError("%s is not a valid value for reduction" % (reduction,))
        if int(blank) < 0:
            raise ValueError("blank must be >= 0, got %d" % int(blank))
        self.blank = int(blank)
        self.reduction = reduction
        self.zero_infinity = bool(zero_infinity)

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ops.ctc_loss(log_probs, targets, input_lengths, target_lengths, self.blank, self.reduction, self.zero_infinity)


class Embedding(_tnn.Embedding):
    """nn.Embedding(num_embeddings, embedding_dim, padding_idx=None): a row lookup whose backward is deterministic (per table row the sum of
    its gradient rows in ascending position).  max_norm, sparse and scale_grad_by_freq are refused."""

    def forward(self, ids):
        if self.max_norm is not None or self.sparse or self.scale_grad_by_freq:
            raise NotImplementedError("ctc_pytorch_amd.nn.Embedding: max_norm, sparse and scale_grad_by_freq are not supported")
        ops._need_gpu(self.weight)
        if torch.is_tensor(ids):
            ops._need_gpu(ids)
        return ops.embedding(ids, self.weight, self.padding_idx)


class CrossEntropyLoss(_tnn.Module):
    """nn.CrossEntropyLoss(ignore_index=-100, reduction='mean') for class-index targets: input (N, C) logits (or (C,) with a 0-d target),
    reduction 'none' / 'sum' / 'mean' (over the rows not ignored).  weight, label_smoothing != 0 and probability targets are refused."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if weight is not None or size_average is not None or reduce is not None:
            raise NotImplementedError("ctc_pytorch_amd.nn.CrossEntropyLoss: class weights and the legacy size_average / reduce are not supported")
        if float(label_smoothing) != 0.0:
            raise NotImplementedError("ctc_pytorch_amd.nn.CrossEntropyLoss: label_smoothing must be 0")
        if reduction not in ("none", "sum", "mean"):
            raise ValueError("%s is not a valid value for reduction" % (reduction,))
        self.ignore_index = int(ignore_index)
        self.reduction = reduction

    def forward(self, input, target):
        if torch.is_tensor(target) and target.is_floating_point():
            raise NotImplementedError("ctc_pytorch_amd.nn.CrossEntropyLoss: class-index targets only (no class probabilities)")
        ops._need_gpu(input)
        if torch.is_tensor(target):
            ops._need_gpu(target)
        if input.dim() not in (1, 2):
            raise NotImplementedError("ctc_pytorch_amd.nn.CrossEntropyLoss: input must be (N, C) or (C,)")
        return ops.cross_entropy(input, target, self.ignore_index, self.reduction)


class MaxPool2d(_tnn.Module):
    """nn.MaxPool2d(pooling_size) of LayerCNN (model_ctc.py:52-53): stride = kernel, no padding, floor."""

    def __init__(self, kernel_size, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False):
        super().__init__()
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        st = ks if stride is None else ((stride, stride) if isinstance(stride, int) else tuple(stride))
        if st != ks or padding not in (0, (0, 0)) or dilation not in (1, (1, 1)) or return_indices or ceil_mode:
            raise NotImplementedError("MaxPool2d(kernel_size) with its defaults only (model_ctc.py:53)")
        self.kernel_size = ks

    def forward(self, x):
        return ops.max_pool2d(x, self.kernel_size)

    def extra_repr(self):
        return "kernel_size=%s" % (self.kernel_size,)


class Conv1d(_tnn.Conv1d):
    """nn.Conv1d of LayerCNN's one-element kernel_size branch (model_ctc.py:48-50): (B,Ci,L) -> (B,Co,L').  Runs on the Conv2d kernels as
    an image of height 1 (kernel (1,k), stride (1,s), padding (0,p)): the fma chain of an output element is the same one, and the parameter
    keeps nn.Conv1d's (Co,Ci,k) shape, so state_dicts are interchangeable with the reference's."""

    def forward(self, x):
        if self.groups != 1 or tuple(self.dilation) != (1,) or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise NotImplementedError("plain Conv1d (groups=1, dilation=1, zero padding) only (model_ctc.py:49)")
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError("Conv1d expects (B,C,L)")          # (a 4-D input -- what CTC_Model.forward feeds -- is refused by torch as well)
        y = ops.conv2d(ops.contiguous(x).unsqueeze(2), self.weight.unsqueeze(2), self.bias, (1, self.stride[0]), (0, self.padding[0]))
        return y.squeeze(2)


class MaxPool1d(_tnn.Module):
    """nn.MaxPool1d(pooling_size) of LayerCNN (model_ctc.py:54-55): stride = kernel, no padding, floor; (B,C,L) -> (B,C,L // k)."""

    def __init__(self, kernel_size, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False):
        super().__init__()
        if isinstance(kernel_size, (tuple, list)):
            (kernel_size,) = kernel_size
        if (stride not in (None, kernel_size, (kernel_size,))) or padding not in (0, (0,)) or dilation not in (1, (1,)) or return_indices or ceil_mode:
            raise NotImplementedError("MaxPool1d(kernel_size) with its defaults only (model_ctc.py:55)")
        self.kernel_size = kernel_size          # (None constructs, as in torch -- LayerCNN builds MaxPool1d(None) for pooling_size=None -- and fails in forward)

    def forward(self, x):
        if self.kernel_size is None:
            raise TypeError("MaxPool1d: kernel_size is None (LayerCNN's one-element kernel_size branch needs a pooling_size, model_ctc.py:54-55)")
        if x.dim() != 3:
            raise ValueError("MaxPool1d expects (B,C,L)")
        return ops.max_pool2d(ops.contiguous(x).unsqueeze(2), (1, int(self.kernel_size))).squeeze(2)

    def extra_repr(self):
        return "kernel_size=%s" % (self.kernel_size,)
