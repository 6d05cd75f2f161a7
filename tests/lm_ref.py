"""Restatement of the kernels of lm.hip and of models/model_rnnlm.RNNLM in numpy / torch on the CPU  --  TEST INFRASTRUCTURE ONLY (used by
test_lm_kernels.py, test_rnnlm.py, test_rnnlm_host.py).

Bit-level definitions (what the C ABI of include/ctcn.h promises; the tests compare bits):
  embedding_fwd   a row copy; zeros for the padding id and for ids outside [0, V), which raise status bit 1.
  embedding_bwd   per table row v: s = dy[n0]; s = fl32(s + dy[n1]); ... over the rows n0 < n1 < ... with ids[n] == v (ids outside [0, V) and
                  the padding id name no row); beta = 0: the row is s (zeros for an empty list); beta = 1: fl32(dtable[v] + s), and dtable[v]
                  untouched for an empty list.
  nll             tok = -lp[n, tgt[n]] (float32; 0 for ignored rows and for targets outside [0, V), the latter raising status bit 2);
                  seq_sum[b] = float64 sum over t ascending from 0.0; total = float64 sum over b ascending from 0.0; count = rows whose target
                  is not ignore_index.
  pack / select   integers, and float64 with every product and sum rounded on its own (numpy float64 scalars do exactly that).
Bounded definition:
  xent_bwd        dz = g_n (exp(lp) - onehot), evaluated here in float64 from the SAME float32 lp bits; xent_bound() is the per-element
                  bound on the kernel's float32 result (its derivation is in the function's docstring).
"""
import numpy as np
import torch
import torch.nn as tnn
import torch.nn.functional as F

U = 2.0 ** -24                 # float32 unit roundoff
IGNORE = -100
BOUNDARY = 0


def embedding_fwd(ids, table, padding_idx=-1):
    ids = np.asarray(ids).reshape(-1)
    V, E = table.shape
    y = np.zeros((ids.size, E), dtype=table.dtype)
    status = 0
    for n, k in enumerate(ids):
        if k == padding_idx and padding_idx >= 0:
            continue
        if k < 0 or k >= V:
            status |= 1
            continue
        y[n] = table[k]
    return y, status


def embedding_bwd(ids, dy, dtable, padding_idx=-1, beta=0.0, dtype=np.float32):
    """The ascending-n loop in `dtype` additions; returns the new table gradient."""
    ids = np.asarray(ids).reshape(-1)
    dy = np.asarray(dy, dtype=dtype)
    V, E = dtable.shape
    out = np.array(dtable, dtype=dtype, copy=True) if beta != 0 else np.zeros((V, E), dtype=dtype)
    sums, seen = np.zeros((V, E), dtype=dtype), np.zeros(V, dtype=bool)
    for n, k in enumerate(ids):
        if k < 0 or k >= V or k == padding_idx:
            continue
        if seen[k]:
            sums[k] = (sums[k] + dy[n]).astype(dtype)
        else:
            sums[k], seen[k] = dy[n], True
    for v in range(V):
        if seen[v]:
            out[v] = (dtype(beta) * out[v] + sums[v]).astype(dtype) if beta != 0 else sums[v]
        elif beta != 0:
            out[v] = (dtype(beta) * out[v]).astype(dtype)
    return out


def nll(lp, tgt, T, B, ignore_index=IGNORE):
    """lp (T*B, V) float32, tgt (T*B): (tok float32 (T*B), seq_sum float64 (B), total float64, count, status)."""
    lp = np.asarray(lp, dtype=np.float32)
    tgt = np.asarray(tgt).reshape(-1)
    V = lp.shape[1]
    tok = np.zeros(T * B, dtype=np.float32)
    status = 0
    for n, k in enumerate(tgt):
        if k == ignore_index:
            continue
        if k < 0 or k >= V:
            status |= 2
            continue
        tok[n] = -lp[n, k]
    seq = np.zeros(B, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            seq = seq + tok[t * B:(t + 1) * B].astype(np.float64)
        total = np.float64(0.0)
        for b in range(B):
            total = total + seq[b]
    return tok, seq, total, int((tgt != ignore_index).sum()), status


def xent_bwd(lp, tgt, g, g_stride, count=None, ignore_index=IGNORE):
    """float64 dz from float32 lp bits: g_n (exp(lp) - onehot), g_n = g[n * g_stride] (/ max(count, 1)); zeros for dead rows.
    Returns (dz, p, y, gn) -- the probabilities, the one-hot rows and the row scales, for xent_bound."""
    lp64 = np.asarray(lp, dtype=np.float32).astype(np.float64)
    tgt = np.asarray(tgt).reshape(-1)
    N, V = lp64.shape
    g = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64)
    live = (tgt != ignore_index) & (tgt >= 0) & (tgt < V)
    gn = np.where(live, g[np.arange(N) * g_stride], 0.0)
    if count is not None:
        gn = gn / max(int(count), 1)
    with np.errstate(under="ignore"):
        p = np.exp(lp64)
    y = np.zeros((N, V))
    y[np.arange(N)[live], tgt[live]] = 1.0
    p, y = p * live[:, None], y * live[:, None]
    return gn[:, None] * (p - y), p, y, gn


def xent_bound(p, y, gn, mean):
    """Per-element bound on |dz_kernel - dz_float64| for dz = fl(g_n * fl(expf(lp) - y)), u = 2^-24:
      expf      float32 expf is within 1 ulp, a relative error of at most 2 u: |e - p| <= 2 u p (plus a result in the subnormal range,
                flushed or rounded there: at most 2^-126 absolute)
      subtract  fl(e - y) = (e - y)(1 + d), |d| <= u: the rounding adds at most u |e - y| <= u (|p - y| + 2 u p)
      g_n       'mean' divides the float32 upstream gradient by the float32 count: one rounding, u |g_n|; otherwise g_n is exact
      product   one rounding, u of the product
    Together |error| <= |g_n| (2 u p + (2 + m) u |p - y|) (1 + 4 u) + |g_n| 2^-126 + 2^-149 with m = 1 for 'mean' -- the last term is the
    product's own underflow.  Rows that are ignored have p = y = g_n = 0 here: their bound is 2^-149 and the kernel writes exact zeros."""
    m = 1.0 if mean else 0.0
    a = np.abs(gn)[:, None]
    return a * (2 * U * p + (2 + m) * U * np.abs(p - y)) * (1 + 4 * U) + a * 2.0 ** -126 + 2.0 ** -149


def pack_nbest(out_ids, out_len, count, L, boundary=BOUNDARY, ignore_index=IGNORE):
    B, N, T = out_ids.shape
    S = B * N
    ids = np.zeros((L + 1, S), dtype=np.int32)
    tgt = np.full((L + 1, S), ignore_index, dtype=np.int32)
    lens = np.zeros(S, dtype=np.int32)
    for b in range(B):
        for k in range(N):
            s = b * N + k
            n = min(max(int(out_len[b, k]), 0), min(L, T)) if k < count[b] else 0
            y = out_ids[b, k, :n]
            ids[0, s] = boundary
            ids[1:n + 1, s] = y
            tgt[:n, s] = y
            tgt[n, s] = boundary
            lens[s] = n + 1
    return ids, tgt, lens


def rescore_select(score, lm, out_len, count, out_ids, weight, len_bonus):
    B, N, T = out_ids.shape
    best_ids = np.zeros((B, T), dtype=np.int32)
    best_len = np.zeros(B, dtype=np.int32)
    best_score = np.zeros(B, dtype=np.float64)
    best_k = np.full(B, -1, dtype=np.int32)
    w, lb = np.float64(weight), np.float64(len_bonus)
    for b in range(B):
        for k in range(min(max(int(count[b]), 0), N)):
            t = (np.float64(score[b, k]) + w * np.float64(lm[b, k])) + lb * np.float64(out_len[b, k])
            if best_k[b] < 0 or t > best_score[b]:
                best_k[b], best_score[b] = k, t
        if best_k[b] >= 0:
            n = min(max(int(out_len[b, best_k[b]]), 0), T)
            best_len[b] = n
            best_ids[b, :n] = out_ids[b, best_k[b], :n]
    return best_ids, best_len, best_score, best_k


def lm_batch(labellings, boundary=BOUNDARY, ignore_index=IGNORE):
    """The host batch of a list of labellings (the rule of ctcn_lm_pack_nbest): ids, targets (L+1, B) int64 and lens (B)."""
    B, L = len(labellings), max(len(r) for r in labellings)
    ids = np.zeros((L + 1, B), dtype=np.int64)
    tgt = np.full((L + 1, B), ignore_index, dtype=np.int64)
    lens = np.zeros(B, dtype=np.int64)
    for b, r in enumerate(labellings):
        n = len(r)
        ids[0, b] = boundary
        ids[1:n + 1, b] = r
        tgt[:n, b] = r
        tgt[n, b] = boundary
        lens[b] = n + 1
    return ids, tgt, lens


class _OracleBlock(tnn.Module):
    def __init__(self, input_size, hidden_size, rnn_type, batch_norm):
        super().__init__()
        self.batch_norm = tnn.BatchNorm1d(input_size) if batch_norm else None
        self.rnn = rnn_type(input_size=input_size, hidden_size=hidden_size, bidirectional=False, bias=False)


def _bn_valid(bn, x, mask):
    """BatchNorm over the real positions x[mask] only, zeros elsewhere (tests/packed_ref.py)."""
    rows = x[mask]
    if bn.training:
        bn.num_batches_tracked += 1
    y = F.batch_norm(rows, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)
    out = torch.zeros_like(x)
    out[mask] = y
    return out


class OracleRNNLM(tnn.Module):
    """RNNLM from torch's own modules on the CPU: same module tree, same state_dict keys; BatchNorms see the real positions only and the
    recurrences run over packed sequences.  `dtype` (float32 / float64) via .to(dtype)."""

    def __init__(self, num_class, emb_size, hidden_size, layers, rnn_type=tnn.LSTM, batch_norm=True):
        super().__init__()
        self.num_class = num_class
        self.embed = tnn.Embedding(num_class, emb_size)
        self.rnns = tnn.Sequential(*[_OracleBlock(emb_size if n == 0 else hidden_size, hidden_size, rnn_type, bool(n) and batch_norm)
                                     for n in range(layers)])
        head = tnn.Linear(hidden_size, num_class, bias=False)
        self.fc = tnn.Sequential(tnn.BatchNorm1d(hidden_size), head) if batch_norm else head

    def forward(self, ids_tb, lengths):
        from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
        ids = torch.as_tensor(np.asarray(ids_tb), dtype=torch.int64)
        lens = torch.as_tensor(np.asarray(lengths), dtype=torch.int64)
        T, B = ids.shape
        mask = (torch.arange(T)[None, :] < lens[:, None]).t()            # (T, B)
        h = self.embed(ids)
        for blk in self.rnns:
            h = _bn_valid(blk.batch_norm, h, mask) if blk.batch_norm is not None else torch.where(mask[..., None], h, torch.zeros((), dtype=h.dtype))
            y, _ = blk.rnn(pack_padded_sequence(h, lens, enforce_sorted=False))
            h, _ = pad_packed_sequence(y, total_length=T)
        if isinstance(self.fc, tnn.Sequential):
            z = self.fc[1](_bn_valid(self.fc[0], h, mask).reshape(T * B, -1))
        else:
            z = self.fc(torch.where(mask[..., None], h, torch.zeros((), dtype=h.dtype)).reshape(T * B, -1))
        return z.view(T, B, self.num_class)

    def loss(self, labellings, reduction="mean"):
        ids, tgt, lens = lm_batch(labellings)
        z = self.forward(ids, lens)
        return F.cross_entropy(z.reshape(-1, self.num_class), torch.from_numpy(tgt).reshape(-1), ignore_index=IGNORE, reduction=reduction)

    def score(self, labellings):
        """ln P(y, boundary) per labelling: the float64 sum of the token log-probs."""
        ids, tgt, lens = lm_batch(labellings)
        with torch.no_grad():
            lp = F.log_softmax(self.forward(ids, lens).double(), dim=-1)
        t = torch.from_numpy(tgt)
        tok = torch.gather(lp, 2, t.clamp(min=0)[..., None])[..., 0]
        return torch.where(t == IGNORE, torch.zeros((), dtype=torch.float64), tok).sum(0).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# The learning test's source and the oracle's training loop
def markov_source(K=8, sharp=0.85):
    """A first-order Markov source over K symbols: from symbol i the successor (i + 1) % K with probability `sharp`, the other K - 1 share
    the rest.  Returns (P (K,K), conditional entropy H(X_t | X_t-1), unigram entropy of the stationary distribution), in nats."""
    P = np.full((K, K), (1.0 - sharp) / (K - 1))
    for i in range(K):
        P[i, (i + 1) % K] = sharp
    w, v = np.linalg.eig(P.T)
    pi = np.real(v[:, np.argmin(np.abs(w - 1.0))])
    pi = pi / pi.sum()
    cond = float(-(pi[:, None] * P * np.log(P)).sum())
    uni = float(-(pi * np.log(pi)).sum())
    return P, cond, uni


def sample_sentences(P, n, rng, lo=12, hi=24, first_id=1):
    """n sentences of lo .. hi symbols from the source, symbol k as class id first_id + k (class 0 stays the boundary)."""
    K = P.shape[0]
    out = []
    for _ in range(n):
        s = [rng.randint(K)]
        for _ in range(rng.randint(lo, hi + 1) - 1):
            s.append(int(rng.choice(K, p=P[s[-1]])))
        out.append([first_id + k for k in s])
    return out


def train_oracle(model, train, dev, batches, epochs, lr):
    """Adam on the oracle model over the minibatches `batches(epoch)` (lists of sentence indices) -> dev cross-entropy per token per epoch."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    tokens = sum(len(s) + 1 for s in dev)
    history = []
    for epoch in range(1, epochs + 1):
        model.train()
        for batch in batches(epoch):
            loss = model.loss([train[i] for i in batch], "mean")
            opt.zero_grad()
            loss.backward()
            opt.step()
        model.eval()
        with torch.no_grad():
            history.append(float(model.loss(dev, "sum")) / tokens)
    return history
