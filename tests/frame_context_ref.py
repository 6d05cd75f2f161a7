"""numpy restatement of the delta stage of ctcn_frame_context (include/ctcn.h) and the host loader path the rest of it is held to.

Deltas are Kaldi's DeltaFeatures (feature-functions): the scales are built in float32 exactly as its constructor builds them; `deltas64` is
the kernel's definition (ascending float64 sum, one rounding), `deltas_kaldi32` Kaldi's own arithmetic (a zeroed float32 row, one AddVec per
offset in ascending order).  Splice, skip, pad and the collate have no restatement here: the yardstick is utils/data_loader itself
(make_context, skip_feat, the pad of SpeechDataset.__getitem__, create_input), which tests/test_host_logic.py pins to the reference's
fixtures; `host_path` / `host_batch` call it.  `host_twin` runs ctcn_frame_context_host, the library's own host form, over one utterance."""
import ctypes

import numpy as np
import torch

from ctc_pytorch_amd import _lib
from ctc_pytorch_amd.utils import data_loader as DL

SETTINGS = [(0, 0, 1, 1), (0, 2, 2, 2), (3, 3, 1, 1), (2, 1, 3, 4), (5, 5, 7, 1)]     # (left, right, skip, n_downsample); the second is shipped


def delta_scales(order, window):
    """[scales_0 .. scales_order], float32, by DeltaFeatures' loops: float32 multiply, float32 add, then a scale by float32(1.0 / sum j^2)."""
    scales = [np.ones(1, dtype=np.float32)]
    for i in range(1, order + 1):
        prev = scales[-1]
        prev_offset = (prev.shape[0] - 1) // 2
        cur_offset = prev_offset + window
        cur = np.zeros(prev.shape[0] + 2 * window, dtype=np.float32)
        normalizer = np.float32(0.0)
        for j in range(-window, window + 1):
            normalizer = np.float32(normalizer + np.float32(j * j))
            for k in range(-prev_offset, prev_offset + 1):
                cur[j + k + cur_offset] = np.float32(cur[j + k + cur_offset] + np.float32(np.float32(j) * prev[k + prev_offset]))
        cur = (cur * np.float32(1.0 / float(normalizer))).astype(np.float32)
        scales.append(cur)
    return scales


def _terms(x, scale, t_idx):
    """Yields (scale_j, rows x[clamp(t + j)]) over the non-zero entries in ascending offset."""
    T = x.shape[0]
    reach = (scale.shape[0] - 1) // 2
    for j in range(-reach, reach + 1):
        s = scale[j + reach]
        if s != 0.0:
            yield s, x[np.clip(t_idx + j, 0, T - 1)]


def deltas64(x, order, window):
    """(T, F (order + 1)) float32: [static | order 1 | order 2], every delta the ascending float64 sum of float32 scale x float32 value (each
    product exact in float64), rounded once."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    T, F = x.shape
    out = np.zeros((T, F * (order + 1)), dtype=np.float32)
    out[:, :F] = x
    if T == 0:
        return out
    t_idx = np.arange(T)
    for i, scale in enumerate(delta_scales(order, window)[1:], 1):
        acc = np.zeros((T, F), dtype=np.float64)
        for s, rows in _terms(x, scale, t_idx):
            acc += np.float64(s) * rows.astype(np.float64)
        out[:, i * F:(i + 1) * F] = acc.astype(np.float32)
    return out


def deltas_kaldi32(x, order, window):
    """Kaldi's arithmetic: output rows start at zero, `AddVec(scale, row)` per offset: out = float32(out + float32(scale * value)).
    Returns (out, bound): bound = n_terms * 2^-24 * sum |scale_j x_j| per element, the worst case of a float32 sum of n_terms products
    (a term is rounded once as a product and once more when it is added -- the first addition, to zero, is exact: n_terms roundings
    along the longest chain, each at most 2^-24 of a quantity that the sum of magnitudes bounds); n_terms counts the non-zero scales."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    T, F = x.shape
    out = np.zeros((T, F * (order + 1)), dtype=np.float32)
    bound = np.zeros((T, F * (order + 1)), dtype=np.float64)
    out[:, :F] = x
    if T == 0:
        return out, bound
    t_idx = np.arange(T)
    for i, scale in enumerate(delta_scales(order, window)[1:], 1):
        acc = np.zeros((T, F), dtype=np.float32)
        mag = np.zeros((T, F), dtype=np.float64)
        n = 0
        for s, rows in _terms(x, scale, t_idx):
            acc = (acc + (np.float32(s) * rows).astype(np.float32)).astype(np.float32)
            mag += np.abs(np.float64(s) * rows.astype(np.float64))
            n += 1
        out[:, i * F:(i + 1) * F] = acc
        bound[:, i * F:(i + 1) * F] = n * 2.0 ** -24 * mag
    return out, bound


def context_frames(T, skip, nd):
    """The loader's arithmetic: len(feature[::skip]) padded to a multiple of n_downsample as SpeechDataset.__getitem__ pads."""
    kept = T if skip in (0, 1) else len(range(0, T, skip))
    if kept % nd != 0:
        kept += nd - kept % nd
    return kept


def host_path(x, left, right, skip, nd):
    """One utterance through the host loader: make_context, skip_feat and the pad of SpeechDataset.__getitem__ (its own statements)."""
    feat = DL.skip_feat(DL.make_context(np.ascontiguousarray(x, dtype=np.float32), left, right, as_view=True), skip)
    seq_len, dim = feat.shape
    if seq_len % nd != 0:
        pad_len = nd - seq_len % nd
        feat = np.vstack([feat, np.zeros((pad_len, dim), dtype=feat.dtype)])
    return np.ascontiguousarray(feat)


def host_batch(utts, left, right, skip, nd, pad_to=None):
    """create_input over host_path of every utterance: (inputs (B, Tmax, F2) float32, fractions (B) float32) as numpy arrays.  pad_to: a
    base frame count the batch is padded to (an empty extra utterance's worth: Tmax becomes context_frames(pad_to))."""
    mats = [host_path(u, left, right, skip, nd) for u in utts]
    items = [(torch.from_numpy(m), torch.zeros(1, dtype=torch.long), "u%d" % i) for i, m in enumerate(mats)]
    if pad_to is not None:
        width = mats[0].shape[1]
        items.append((torch.zeros((context_frames(pad_to, skip, nd), width)), torch.zeros(1, dtype=torch.long), "pad"))
    data, sizes, _, _, _ = DL.create_input(items)
    n = len(utts)
    return data.numpy()[:n], sizes.numpy()[:n], np.array([m.shape[0] for m in mats], dtype=np.int32)


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_twin(x, left=0, right=0, skip=1, nd=1, order=0, window=2, out_rows=None):
    """ctcn_frame_context_host over one utterance: (out (out_rows, F2), n_out, fraction); the rows behind the buffer stay untouched."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    T, F = x.shape
    opts = _lib.ContextOpts(left=left, right=right, skip=skip, n_downsample=nd, delta_order=order, delta_window=window)
    n_out = context_frames(T, skip, nd)
    rows = n_out if out_rows is None else out_rows
    F2 = (left + 1 + right) * F * (order + 1)
    out = np.full((rows + 2, F2), -12345.0, dtype=np.float32)
    frac = np.full(1, -1.0, dtype=np.float32)
    r = _lib.lib().ctcn_frame_context_host(vp(x), T, F, ctypes.byref(opts), vp(out), rows, vp(frac))
    assert r == n_out, (r, n_out, _lib.lib().ctcn_last_error())
    assert np.all(out[rows:] == -12345.0)
    return out[:rows], r, frac[0]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
