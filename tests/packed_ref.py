"""Length-aware torch-CPU reference  --  TEST INFRASTRUCTURE ONLY (used by test_length_mask*.py).

oracle/torch_cpu.py's TorchCpuCTCModel (same modules, same state-dict keys) with the padding kept out of everything:
  * pack_padded_sequence(enforce_sorted=False) / pad_packed_sequence around every RNN;
  * BatchNorm statistics over the valid frames only (the valid rows are gathered, F.batch_norm runs on them with the module's own
    parameters and running statistics, the result is scattered back into zeros);
  * the input of every conv block and its output (after the pooling) are zero at padded frames.
Frames per stage: conv floor((len + 2 p_t - k_t) / s_t) + 1, time pooling floor(len / pool_t).
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import torch_cpu


def time_mask(lens, T):
    """(B, T) bool: frame t of utterance b is real."""
    return torch.arange(T)[None, :] < lens[:, None]


def _bn_valid(bn, x, mask):
    """BatchNorm over x[mask] (mask indexes the leading dims of x; channels are dim 1 of the gathered rows), zeros elsewhere."""
    rows = x[mask]
    if bn.training:
        bn.num_batches_tracked += 1
    y = F.batch_norm(rows, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)
    out = torch.zeros_like(x)
    out[mask] = y
    return out


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def conv_block_lengths(blk, lens):
    k, s, p = blk.conv.kernel_size[0], blk.conv.stride[0], blk.conv.padding[0]
    after_conv = (lens + 2 * p - k) // s + 1
    pool_t = _pair(blk.pooling.kernel_size)[0] if blk.pooling is not None else 1
    return after_conv, after_conv // pool_t


def _zero_padded(x, mask):
    """x (B, T, ...) with the padded frames replaced by zeros (select: NaN in the padding does not propagate)."""
    m = mask.view(mask.shape + (1,) * (x.dim() - 2))
    return torch.where(m, x, torch.zeros((), dtype=x.dtype))


class PackedCpuCTCModel(torch_cpu.TorchCpuCTCModel):
    def output_lengths(self, input_lengths):
        lens = torch.as_tensor(np.asarray(input_lengths), dtype=torch.int64)
        if self.add_cnn:
            for blk in self.conv:
                lens = conv_block_lengths(blk, lens)[1]
        return lens

    def forward(self, x, input_lengths):
        lens = torch.as_tensor(np.asarray(input_lengths), dtype=torch.int64)
        B, T, _ = x.shape
        h = _zero_padded(x, time_mask(lens, T))
        if self.add_cnn:
            c = h.unsqueeze(1)                                          # (B,1,T,F)
            for blk in self.conv:
                c = blk.conv(c)
                len_conv, len_pool = conv_block_lengths(blk, lens)
                ct = c.transpose(1, 2)                                  # (B,T',C,F'): frames lead, channels are dim 1 of a gathered row
                m = time_mask(len_conv, ct.shape[1])
                ct = _bn_valid(blk.batch_norm, ct, m) if blk.batch_norm is not None else _zero_padded(ct, m)
                c = blk.activation(ct.transpose(1, 2).contiguous())
                if blk.pooling is not None:
                    c = blk.pooling(c)
                    c = _zero_padded(c.transpose(1, 2), time_mask(len_pool, c.shape[2])).transpose(1, 2)
                c = blk.dropout(c)
                lens = len_pool
            h = c.transpose(1, 2).contiguous()
            h = h.view(h.size(0), h.size(1), -1).transpose(0, 1).contiguous()
        else:
            h = h.transpose(0, 1)
        Tp = h.shape[0]
        m_tb = time_mask(lens, Tp).t()                                  # (T',B)
        for blk in self.rnns:
            if blk.batch_norm is not None:
                h = _bn_valid(blk.batch_norm, h, m_tb)
            packed = pack_padded_sequence(h, lens, enforce_sorted=False)
            y, _ = blk.rnn(packed)
            h, _ = pad_packed_sequence(y, total_length=Tp)
            h = blk.dropout(h)
        if isinstance(self.fc, torch.nn.Sequential):
            z = self.fc[1](_bn_valid(self.fc[0], h, m_tb).reshape(Tp * B, -1))
        else:
            z = self.fc(_zero_padded(h.transpose(0, 1), m_tb.t()).transpose(0, 1).reshape(Tp * B, -1))
        return self.log_softmax(z.view(Tp, B, -1))
