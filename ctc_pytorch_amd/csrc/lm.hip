// lm.hip -- the kernels of the RNN language model and of n-best rescoring (ctcn_embedding_fwd / _bwd, ctcn_nll_fwd, ctcn_xent_bwd,
// ctcn_lm_pack_nbest, ctcn_rescore_select; contract in include/ctcn.h).  The recurrent stack, BatchNorm, the output product and the
// log-softmax of the model are the acoustic model's kernels; what is here is what sits in front of and behind them.
//
// embedding_fwd_kernel: one wave per row, lanes across the columns (16 bytes per lane where table, y and E allow it).  The id is checked
//   before it indexes anything; a padding or out-of-range row is written as zeros without a read.
// ctcn_embedding_bwd: a scatter-add without float atomics, the sum per table row in ascending n:
//   1 emb_rank_kernel    per chunk of 256 rows: every row's rank among the rows of the same id in its chunk (a scan over the chunk's ids in
//                        LDS, a broadcast read per step); the last row of an id writes the id's count for the chunk
//   2 emb_chunk_scan     per id: exclusive prefix over the chunks of those counts (a thread per id, coalesced over ids), the total per id
//   3 emb_id_scan        one workgroup: exclusive prefix of the totals over the ids = where each id's list starts
//   4 emb_place_kernel   per row: perm[start[id] + prefix[chunk][id] + rank] = n -- a stable counting sort, every slot written once
//   5 emb_sum_kernel     one wave per (id, 64 or 256 columns): walks the id's list in order, eight row loads in flight (the addresses come
//                        from perm, which is wave-uniform: scalar loads), the additions in list order
//   Lists are not split, whatever their length: the order of the additions is the definition of the result.
// nll: tok by a thread per row; the per-sequence sums by a thread per sequence (coalesced over b, ascending t); the total and the count by
//   one workgroup (the count is an integer sum: any order; the total is thread 0's loop in ascending b).
// xent_bwd_kernel: V <= XENT_WAVE_MAX_V: one wave per row, four rows per workgroup; above: one workgroup of 256 threads per row.  One read of
//   lp, one write of dz, 16 bytes per lane where lp, dz and V allow it.  The row's gradient scale is formed once per row.
// pack / select: a thread per element of the LM's batch; a wave per utterance, lane 0 choosing, all lanes copying the winner's ids.
#include "common.h"

// Every product, sum and quotient below is rounded on its own (the contract of include/ctcn.h): nothing in this file may be compiled into
// fused multiply-adds.
#pragma clang fp contract(off)

namespace {

constexpr int EMB_CHUNK = 256;                     // rows per chunk of the counting sort (= threads of its kernels)
constexpr int XENT_WAVE_MAX_V = 512;               // widest row a single wave takes in xent_bwd_kernel
constexpr int LM_MAX_ROWS = 1 << 30;

__device__ __forceinline__ bool aligned16(const void *a, const void *b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

__global__ __launch_bounds__(256) void embedding_fwd_kernel(const int32_t *__restrict__ ids, const float *__restrict__ table, float *__restrict__ y,
                                                            int N, int V, int E, int padding_idx, int32_t *status) {
  const int lane = threadIdx.x & 63;
  const size_t n = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= (size_t)N) return;
  const int id = ids[n];
  const bool bad = id < 0 || id >= V;
  const bool pad = id == padding_idx && padding_idx >= 0;
  if (bad && !pad && lane == 0) atomicOr(status, 1);
  const float *src = table + (size_t)(bad ? 0 : id) * E;
  float *dst = y + n * E;
  const bool zero = bad || pad;
  if ((E & 3) == 0 && aligned16(table, y)) {
    for (int c = lane * 4; c < E; c += 256) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!zero) v = *reinterpret_cast<const float4 *>(src + c);
      *reinterpret_cast<float4 *>(dst + c) = v;
    }
  } else {
    for (int c = lane; c < E; c += 64) dst[c] = zero ? 0.f : src[c];
  }
}

__device__ __forceinline__ int emb_valid_id(const int32_t *__restrict__ ids, int n, int N, int V, int padding_idx) {
  if (n >= N) return -1;
  const int id = ids[n];
  return (id < 0 || id >= V || id == padding_idx) ? -1 : id;
}

__global__ __launch_bounds__(EMB_CHUNK) void emb_rank_kernel(const int32_t *__restrict__ ids, int N, int V, int padding_idx, int32_t *__restrict__ rank,
                                                             int32_t *__restrict__ hist) {
  __shared__ int sid[EMB_CHUNK];
  const int i = threadIdx.x, c = blockIdx.x, n = c * EMB_CHUNK + i;
  const int id = emb_valid_id(ids, n, N, V, padding_idx);
  sid[i] = id;
  __syncthreads();
  if (id < 0) return;
  int r = 0, later = 0;
  for (int j = 0; j < i; ++j) r += sid[j] == id;
  for (int j = i + 1; j < EMB_CHUNK; ++j) later |= sid[j] == id;
  rank[n] = r;
  if (!later) hist[(size_t)c * V + id] = r + 1;                       // (hist was cleared: an id absent from the chunk counts 0)
}

__global__ __launch_bounds__(256) void emb_chunk_scan(int32_t *__restrict__ hist, int32_t *__restrict__ start, int V, int nchunks) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int run = 0;
  for (int c = 0; c < nchunks; ++c) {
    const int h = hist[(size_t)c * V + v];
    hist[(size_t)c * V + v] = run;
    run += h;
  }
  start[v] = run;
}

__global__ __launch_bounds__(256) void emb_id_scan(int32_t *__restrict__ start, int V) {
  __shared__ int part[256];
  const int t = threadIdx.x, per = (V + 255) / 256;
  const int lo = min(t * per, V), hi = min(lo + per, V);
  int s = 0;
  for (int v = lo; v < hi; ++v) s += start[v];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < 256; ++k) { const int p = part[k]; part[k] = run; run += p; }
    start[V] = run;
  }
  __syncthreads();
  int run = part[t];
  for (int v = lo; v < hi; ++v) { const int cnt = start[v]; start[v] = run; run += cnt; }
}

__global__ __launch_bounds__(EMB_CHUNK) void emb_place_kernel(const int32_t *__restrict__ ids, int N, int V, int padding_idx, const int32_t *__restrict__ rank,
                                                              const int32_t *__restrict__ hist, const int32_t *__restrict__ start, int32_t *__restrict__ perm) {
  const int c = blockIdx.x, n = c * EMB_CHUNK + threadIdx.x;
  const int id = emb_valid_id(ids, n, N, V, padding_idx);
  if (id < 0) return;
  perm[start[id] + hist[(size_t)c * V + id] + rank[n]] = n;           // below start[V] <= N: every valid row has exactly one slot
}

template <int VEC> struct Cols { float x[VEC]; };

template <int VEC> __device__ __forceinline__ Cols<VEC> load_cols(const float *p) {
  Cols<VEC> r;
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    r.x[0] = q.x; r.x[1] = q.y; r.x[2] = q.z; r.x[3] = q.w;
  } else {
    r.x[0] = *p;
  }
  return r;
}

template <int VEC> __device__ __forceinline__ void store_cols(float *p, const Cols<VEC> &r) {
  if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.x[0], r.x[1], r.x[2], r.x[3]);
  else *p = r.x[0];
}

template <int VEC>
__global__ __launch_bounds__(64) void emb_sum_kernel(const float *__restrict__ dy, float *dtable, const int32_t *__restrict__ perm,
                                                     const int32_t *__restrict__ start, int E, float beta) {
  const int v = blockIdx.x, col = (blockIdx.y * 64 + threadIdx.x) * VEC;
  if (col >= E) return;
  const int beg = start[v], end = start[v + 1];
  float *dst = dtable + (size_t)v * E + col;
  Cols<VEC> out;
  if (beta != 0.f) {
    out = load_cols<VEC>(dst);
#pragma unroll
    for (int e = 0; e < VEC; ++e) out.x[e] = beta * out.x[e];
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) out.x[e] = 0.f;
  }
  if (beg < end) {
    const float *src = dy + col;
    Cols<VEC> s = load_cols<VEC>(src + (size_t)perm[beg] * E);
    int p = beg + 1;
    for (; p + 8 <= end; p += 8) {
      Cols<VEC> r[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = load_cols<VEC>(src + (size_t)perm[p + u] * E);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) s.x[e] = s.x[e] + r[u].x[e];
    }
    for (; p < end; ++p) {
      const Cols<VEC> r = load_cols<VEC>(src + (size_t)perm[p] * E);
#pragma unroll
      for (int e = 0; e < VEC; ++e) s.x[e] = s.x[e] + r.x[e];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) out.x[e] = beta != 0.f ? out.x[e] + s.x[e] : s.x[e];
  }
  store_cols<VEC>(dst, out);
}

struct EmbWs { int32_t *rank, *perm, *start, *hist; size_t hist_bytes, total; int nchunks; };

EmbWs emb_ws(void *ws, int N, int V) {
  EmbWs w;
  w.nchunks = ceil_div(N, EMB_CHUNK);
  const size_t n4 = align_up((size_t)N * 4, 16), v4 = align_up(((size_t)V + 1) * 4, 16);
  char *p = (char *)ws;
  w.rank = (int32_t *)p;
  w.perm = (int32_t *)(p + n4);
  w.start = (int32_t *)(p + 2 * n4);
  w.hist = (int32_t *)(p + 2 * n4 + v4);
  w.hist_bytes = (size_t)w.nchunks * V * 4;
  w.total = 2 * n4 + v4 + align_up(w.hist_bytes, 16);
  return w;
}

__global__ __launch_bounds__(256) void nll_tok_kernel(const float *__restrict__ lp, const int32_t *__restrict__ tgt, int N, int V, int ignore_index,
                                                      float *__restrict__ tok, int32_t *status) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int t = tgt[n];
  float r = 0.f;
  if (t != ignore_index) {
    if (t >= 0 && t < V) r = -lp[(size_t)n * V + t];
    else atomicOr(status, 2);
  }
  tok[n] = r;
}

__global__ __launch_bounds__(256) void nll_seq_kernel(const float *__restrict__ tok, int T, int B, double *__restrict__ seq_sum) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
#pragma unroll 8
  for (int t = 0; t < T; ++t) s += (double)tok[(size_t)t * B + b];
  seq_sum[b] = s;
}

__global__ __launch_bounds__(256) void nll_total_kernel(const double *__restrict__ seq_sum, const int32_t *__restrict__ tgt, int N, int B, int ignore_index,
                                                        double *__restrict__ total, int32_t *__restrict__ count) {
  __shared__ int part[4];
  int c = 0;
  for (int n = threadIdx.x; n < N; n += 256) c += tgt[n] != ignore_index;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    *count = part[0] + part[1] + part[2] + part[3];
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += seq_sum[b];
    *total = s;
  }
}

// the threads of one row (a wave, or a workgroup) write dz[n, :]; `tid` / `nthr` are the thread's place among them
template <int NTHR>
__device__ __forceinline__ void xent_row(const float *__restrict__ lp, const int32_t *__restrict__ tgt, float *__restrict__ dz, size_t n, int V,
                                         int ignore_index, const float *__restrict__ g, int g_stride, const int32_t *__restrict__ count, int tid) {
  const int t = tgt[n];
  const bool live = t != ignore_index && t >= 0 && t < V;
  float gn = 0.f;
  if (live) {
    gn = g[n * (size_t)g_stride];
    if (count) gn = gn / (float)max(*count, 1);
  }
  const float *src = lp + n * V;
  float *dst = dz + n * V;
  if ((V & 3) == 0 && aligned16(lp, dz)) {
    for (int c = tid * 4; c < V; c += NTHR * 4) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) {
        const float4 q = *reinterpret_cast<const float4 *>(src + c);
        o.x = gn * (expf(q.x) - (c == t ? 1.f : 0.f));
        o.y = gn * (expf(q.y) - (c + 1 == t ? 1.f : 0.f));
        o.z = gn * (expf(q.z) - (c + 2 == t ? 1.f : 0.f));
        o.w = gn * (expf(q.w) - (c + 3 == t ? 1.f : 0.f));
      }
      *reinterpret_cast<float4 *>(dst + c) = o;
    }
  } else {
    for (int c = tid; c < V; c += NTHR) dst[c] = live ? gn * (expf(src[c]) - (c == t ? 1.f : 0.f)) : 0.f;
  }
}

template <bool WAVE_ROWS>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const float *__restrict__ lp, const int32_t *__restrict__ tgt, float *__restrict__ dz, int N, int V,
                                                       int ignore_index, const float *__restrict__ g, int g_stride, const int32_t *__restrict__ count) {
  if constexpr (WAVE_ROWS) {
    const size_t n = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n < (size_t)N) xent_row<64>(lp, tgt, dz, n, V, ignore_index, g, g_stride, count, threadIdx.x & 63);
  } else {
    xent_row<256>(lp, tgt, dz, blockIdx.x, V, ignore_index, g, g_stride, count, threadIdx.x);
  }
}

__global__ __launch_bounds__(256) void lm_pack_kernel(const int32_t *__restrict__ out_ids, const int32_t *__restrict__ out_len, const int32_t *__restrict__ count,
                                                      int B, int N, int T, int L, int boundary, int ignore_index, int32_t *__restrict__ in_ids,
                                                      int32_t *__restrict__ tgt, int32_t *__restrict__ lens) {
  const int S = B * N;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)(L + 1) * S) return;
  const int t = (int)(i / S), s = (int)(i % S), b = s / N, k = s % N;
  const int l = k < count[b] ? min(max(out_len[s], 0), min(L, T)) : 0;
  const int32_t *y = out_ids + (size_t)s * T;
  in_ids[i] = t == 0 ? boundary : (t <= l ? y[t - 1] : 0);
  tgt[i] = t < l ? y[t] : (t == l ? boundary : ignore_index);
  if (t == 0) lens[s] = l + 1;
}

__global__ __launch_bounds__(64) void rescore_select_kernel(const double *__restrict__ score, const double *__restrict__ lm, const int32_t *__restrict__ out_len,
                                                            const int32_t *__restrict__ count, const int32_t *__restrict__ out_ids, double weight,
                                                            double len_bonus, int N, int T, int32_t *__restrict__ best_ids, int32_t *__restrict__ best_len,
                                                            double *__restrict__ best_score, int32_t *__restrict__ best_k) {
  const int b = blockIdx.x;
  int k_best = -1;
  double t_best = 0.0;
  if (threadIdx.x == 0) {
    const int cnt = min(max(count[b], 0), N);
    for (int k = 0; k < cnt; ++k) {
      const size_t i = (size_t)b * N + k;
      const double t = (score[i] + weight * lm[i]) + len_bonus * (double)out_len[i];
      if (k_best < 0 || t > t_best) { k_best = k; t_best = t; }
    }
    best_k[b] = k_best;
    best_score[b] = t_best;
  }
  k_best = __shfl(k_best, 0, 64);
  const int len = k_best < 0 ? 0 : min(max(out_len[(size_t)b * N + k_best], 0), T);
  if (threadIdx.x == 0) best_len[b] = len;
  const int32_t *src = out_ids + ((size_t)b * N + max(k_best, 0)) * T;
  for (int t = threadIdx.x; t < T; t += 64) best_ids[(size_t)b * T + t] = t < len ? src[t] : 0;
}

}  // namespace

extern "C" int ctcn_embedding_fwd(const int32_t *ids, const float *table, float *y, int N, int V, int E, int padding_idx, int32_t *status, void *stream) {
  CTCN_REQUIRE(ids && table && y && status && N > 0 && N <= LM_MAX_ROWS && V > 0 && E > 0 && padding_idx >= -1,
               "ctcn_embedding_fwd: bad args (N %d at most 2^30, V %d, E %d, padding_idx %d)", N, V, E, padding_idx);
  hipLaunchKernelGGL(embedding_fwd_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, (hipStream_t)stream, ids, table, y, N, V, E, padding_idx, status);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" size_t ctcn_embedding_bwd_ws_bytes(int N, int V) {
  if (N <= 0 || N > LM_MAX_ROWS || V <= 0 || (size_t)ceil_div(N, EMB_CHUNK) * V > ((size_t)1 << 30)) return 0;
  return emb_ws(nullptr, N, V).total;
}

extern "C" int ctcn_embedding_bwd(const int32_t *ids, const float *dy, float *dtable, int N, int V, int E, int padding_idx, float beta, void *ws,
                                  size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(ids && dy && dtable && ws && N > 0 && N <= LM_MAX_ROWS && V > 0 && E > 0 && padding_idx >= -1,
               "ctcn_embedding_bwd: bad args (N %d at most 2^30, V %d, E %d, padding_idx %d)", N, V, E, padding_idx);
  CTCN_REQUIRE(beta == 0.f || beta == 1.f, "ctcn_embedding_bwd: beta must be 0 or 1, got %g", (double)beta);
  CTCN_REQUIRE(((uintptr_t)ws & 3) == 0, "ctcn_embedding_bwd: ws must be 4-byte aligned");
  const size_t need = ctcn_embedding_bwd_ws_bytes(N, V);
  CTCN_REQUIRE(need > 0, "ctcn_embedding_bwd: ceil(N / 256) * V = %zu is beyond 2^30 counters", (size_t)ceil_div(N, EMB_CHUNK) * V);
  if (ws_bytes < need) { ctcn_set_error("ctcn_embedding_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need); return CTCN_EWORKSPACE; }
  const EmbWs w = emb_ws(ws, N, V);
  hipStream_t s = (hipStream_t)stream;
  CTCN_HIP(hipMemsetAsync(w.hist, 0, w.hist_bytes, s));
  hipLaunchKernelGGL(emb_rank_kernel, dim3(w.nchunks), dim3(EMB_CHUNK), 0, s, ids, N, V, padding_idx, w.rank, w.hist);
  hipLaunchKernelGGL(emb_chunk_scan, dim3(ceil_div(V, 256)), dim3(256), 0, s, w.hist, w.start, V, w.nchunks);
  hipLaunchKernelGGL(emb_id_scan, dim3(1), dim3(256), 0, s, w.start, V);
  hipLaunchKernelGGL(emb_place_kernel, dim3(w.nchunks), dim3(EMB_CHUNK), 0, s, ids, N, V, padding_idx, w.rank, w.hist, w.start, w.perm);
  if ((E & 3) == 0 && (((uintptr_t)dy | (uintptr_t)dtable) & 15) == 0) {
    CTCN_REQUIRE(ceil_div(E, 256) <= 65535, "ctcn_embedding_bwd: E %d too wide", E);
    hipLaunchKernelGGL(emb_sum_kernel<4>, dim3(V, ceil_div(E, 256)), dim3(64), 0, s, dy, dtable, w.perm, w.start, E, beta);
  } else {
    CTCN_REQUIRE(ceil_div(E, 64) <= 65535, "ctcn_embedding_bwd: E %d too wide", E);
    hipLaunchKernelGGL(emb_sum_kernel<1>, dim3(V, ceil_div(E, 64)), dim3(64), 0, s, dy, dtable, w.perm, w.start, E, beta);
  }
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_nll_fwd(const float *lp, const int32_t *tgt, int T, int B, int V, int ignore_index, float *tok, double *seq_sum, double *total,
                            int32_t *count, int32_t *status, void *stream) {
  CTCN_REQUIRE(lp && tgt && tok && seq_sum && total && count && status && T > 0 && B > 0 && V > 0 && (long long)T * B <= LM_MAX_ROWS,
               "ctcn_nll_fwd: bad args (T %d, B %d, T * B at most 2^30, V %d)", T, B, V);
  CTCN_REQUIRE((((uintptr_t)seq_sum | (uintptr_t)total) & 7) == 0, "ctcn_nll_fwd: seq_sum and total must be 8-byte aligned");
  const int N = T * B;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nll_tok_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, lp, tgt, N, V, ignore_index, tok, status);
  hipLaunchKernelGGL(nll_seq_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, s, tok, T, B, seq_sum);
  hipLaunchKernelGGL(nll_total_kernel, dim3(1), dim3(256), 0, s, seq_sum, tgt, N, B, ignore_index, total, count);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_xent_bwd(const float *lp, const int32_t *tgt, float *dz, int N, int V, int ignore_index, const float *g, int g_stride,
                             const int32_t *count, void *stream) {
  CTCN_REQUIRE(lp && tgt && dz && g && N > 0 && N <= LM_MAX_ROWS && V > 0 && (g_stride == 0 || g_stride == 1),
               "ctcn_xent_bwd: bad args (N %d at most 2^30, V %d, g_stride %d is 0 or 1)", N, V, g_stride);
  hipStream_t s = (hipStream_t)stream;
  if (V <= XENT_WAVE_MAX_V)
    hipLaunchKernelGGL(xent_bwd_kernel<true>, dim3(ceil_div(N, 4)), dim3(256), 0, s, lp, tgt, dz, N, V, ignore_index, g, g_stride, count);
  else
    hipLaunchKernelGGL(xent_bwd_kernel<false>, dim3(N), dim3(256), 0, s, lp, tgt, dz, N, V, ignore_index, g, g_stride, count);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_lm_pack_nbest(const int32_t *out_ids, const int32_t *out_len, const int32_t *count, int B, int N, int T, int L, int boundary,
                                  int ignore_index, int32_t *in_ids, int32_t *tgt, int32_t *lens, void *stream) {
  CTCN_REQUIRE(out_ids && out_len && count && in_ids && tgt && lens && B > 0 && N > 0 && T > 0 && L >= 0 && L <= T && boundary >= 0 &&
                   (long long)B * N <= (1 << 24) && (long long)B * N * (L + 1) <= LM_MAX_ROWS,
               "ctcn_lm_pack_nbest: bad args (B %d, N %d, T %d, L %d within [0, T], boundary %d; B * N * (L + 1) at most 2^30)", B, N, T, L, boundary);
  const size_t total = (size_t)(L + 1) * B * N;
  hipLaunchKernelGGL(lm_pack_kernel, dim3((unsigned)ceil_div_z(total, 256)), dim3(256), 0, (hipStream_t)stream, out_ids, out_len, count, B, N, T, L,
                     boundary, ignore_index, in_ids, tgt, lens);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_rescore_select(const double *score, const double *lm, const int32_t *out_len, const int32_t *count, const int32_t *out_ids,
                                   double weight, double len_bonus, int B, int N, int T, int32_t *best_ids, int32_t *best_len, double *best_score,
                                   int32_t *best_k, void *stream) {
  CTCN_REQUIRE(score && lm && out_len && count && out_ids && best_ids && best_len && best_score && best_k && B > 0 && N > 0 && T > 0,
               "ctcn_rescore_select: bad args (B %d, N %d, T %d)", B, N, T);
  CTCN_REQUIRE((((uintptr_t)score | (uintptr_t)lm | (uintptr_t)best_score) & 7) == 0, "ctcn_rescore_select: score, lm and best_score must be 8-byte aligned");
  hipLaunchKernelGGL(rescore_select_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, score, lm, out_len, count, out_ids, weight, len_bonus, N, T,
                     best_ids, best_len, best_score, best_k);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
