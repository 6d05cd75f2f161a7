// editops.hip -- the error breakdown behind the error rate: substitutions / deletions / insertions / correct pairs, the alignment itself
// and the confusion table (ctcn_edit_ops; contract in include/ctcn.h).  ctcn_edit_distance (paths.hip) keeps a rolling row and answers the
// distance alone; this kernel keeps the 2-bit move of every cell and walks the chain back.
//
// One wavefront per utterance, the anti-diagonal scheme of edit_distance_wave_kernel (paths.hip): lane L owns the NC reference columns
// L*NC+1 .. (L+1)*NC and at step d fills row i = d - L of them.  Three stages:
//   1. both sequences pass through the class map and are compacted (ballot + popcount, order preserving): the hypothesis into `hyp`, the
//      reference into LDS, from where every lane takes its NC columns into registers;
//   2. the recursion.  Cross-lane traffic per step is two DPP shifts: the right-most cell of the left neighbour (its value of two steps ago is
//      the diagonal) and the hypothesis symbol, which enters at lane 0 and moves one lane per step -- lane 0 takes it from a register that
//      holds 64 symbols (one v_readlane per step, one 64-wide load per 64 steps, fetched a block ahead), so no lane reads memory on the
//      dependent chain.  Every lane packs the moves of its cells, 2 bits each, 16 steps to a word: word ((d >> 4) * NC + c) * 64 + L holds
//      steps 16 * (d >> 4) .. + 15 of column c of lane L -- one conflict-free ds_write_b32 (or one coalesced 256-byte store) per 16 steps;
//   3. lane 0 walks from (nh', nr') back to (0, 0): counts, table entries (vector atomics, integer adds: exact in any order) and, if asked
//      for, the pairs -- written backwards into the END of the utterance's `ali` row, then moved to its front by the whole wave, 64 pairs
//      at a time (a block is read before it is written and lands at or below where it came from), and the rest of the row set to -1.
// Home of `hyp` and the move words (host arithmetic on the shapes alone: the same (lda, max_b_len) always takes the same branch):
//   IN_LDS: dynamic LDS behind the reference (32 x (800 x <= 64): 3.2 + 0.25 + 13.8 KB), the walk pays LDS latency per pair;
//   else  : the caller's workspace, ctcn_edit_ops_ws_bytes (the walk then pays an L2 round trip per pair: the long-label case).
#include <algorithm>

#include "common.h"

namespace {

constexpr size_t EDIT_OPS_LDS_LIMIT = 64 * 1024;     // dynamic LDS of a launch that has not opted in to more (of the CU's 160 KB)

static inline int edit_ops_nc(int max_b_len) { return max_b_len <= 64 ? 1 : max_b_len <= 128 ? 2 : max_b_len <= 256 ? 4 : 8; }
static inline size_t edit_ops_hyp_words(int lda) { return align_up((size_t)std::max(lda, 1), 64); }
// move words of one utterance: steps 1 .. lda + 63, 16 to a word, NC columns, 64 lanes
static inline size_t edit_ops_move_words(int lda, int max_b_len) { return (size_t)(((lda + 63) >> 4) + 1) * edit_ops_nc(max_b_len) * 64; }
static inline size_t edit_ops_ref_words(int max_b_len) { return align_up((size_t)std::max(max_b_len, 1), 64); }
static inline bool edit_ops_in_lds(int lda, int max_b_len) {
  return (edit_ops_ref_words(max_b_len) + edit_ops_hyp_words(lda) + edit_ops_move_words(lda, max_b_len)) * sizeof(uint32_t) <= EDIT_OPS_LDS_LIMIT;
}

// k through the class map: ids outside [0, V) pass through and index nothing; -1 out of the map removes the symbol
__device__ __forceinline__ bool map_symbol(const int32_t *__restrict__ map, int V, int &k) {
  if (map == nullptr || k < 0 || k >= V) return true;
  k = map[k];
  return k != -1;
}

template <int NC, bool IN_LDS>
__global__ __launch_bounds__(64) void edit_ops_wave_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ a_len, const int64_t *__restrict__ bl,
                                                           const int64_t *__restrict__ b_len, const int32_t *__restrict__ map, int V,
                                                           int32_t *__restrict__ counts, int32_t *__restrict__ ali, int32_t *__restrict__ ali_len,
                                                           unsigned long long *__restrict__ conf, int lda, int ldb, int max_b_len,
                                                           uint32_t *__restrict__ ws, size_t ws_words, int ref_words, int hyp_words) {
  extern __shared__ int smem[];
  const int u = blockIdx.x, L = threadIdx.x;
  const int la = min(max(a_len[u], 0), lda), lb = (int)min(max(b_len[u], (int64_t)0), (int64_t)min(max_b_len, ldb));
  const int32_t *pa = a + (size_t)u * lda;
  const int64_t *pb = bl + (size_t)u * ldb;
  int *ref = smem, *hyp;
  uint32_t *moves;
  if constexpr (IN_LDS) {
    hyp = smem + ref_words;
    moves = reinterpret_cast<uint32_t *>(smem + ref_words + hyp_words);
  } else {
    hyp = reinterpret_cast<int *>(ws + (size_t)u * ws_words);
    moves = ws + (size_t)u * ws_words + hyp_words;
  }
  const unsigned long long below = (1ull << L) - 1ull;

  // ---- 1. map + compact ------------------------------------------------------------------------------------------------------------
  int nh = 0, nr = 0;
  for (int t0 = 0; t0 < la; t0 += 64) {
    const int t = t0 + L;
    int k = 0;
    bool keep = false;
    if (t < la) {
      k = pa[t];
      keep = map_symbol(map, V, k);
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) hyp[nh + __popcll(mask & below)] = k;
    nh += __popcll(mask);
  }
  for (int t0 = 0; t0 < lb; t0 += 64) {
    const int t = t0 + L;
    int k = 0;
    bool keep = false;
    if (t < lb) {
      k = (int)pb[t];
      keep = map_symbol(map, V, k);
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) ref[nr + __popcll(mask & below)] = k;
    nr += __popcll(mask);
  }
  if constexpr (!IN_LDS) __threadfence();
  __syncthreads();

  // ---- 2. the recursion, one anti-diagonal per step ----------------------------------------------------------------------------------
  int lab[NC], up[NC];
  uint32_t mv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = L * NC + c + 1;
    lab[c] = j <= nr ? ref[j - 1] : -1;
    up[c] = j;                                          // row 0
    mv[c] = 0u;
  }
  const int last_lane = nr > 0 ? (nr - 1) / NC : 0;     // columns beyond nr feed nothing the walk visits
  const int steps = nh + last_lane;
  int vlast = (L + 1) * NC, left_prev = L * NC, xprev = 0;
  int blk = L < nh ? hyp[L] : 0;                        // hyp[64 * q + L] of the running block q
  for (int d0 = 0; d0 < steps; d0 += 64) {
    const int nxt = d0 + 64 + L < nh ? hyp[d0 + 64 + L] : 0;
    const int dend = min(64, steps - d0);
    for (int s = 0; s < dend; ++s) {
      const int d = d0 + s + 1, i = d - L;
      const bool active = i >= 1 && i <= nh;
      const int x0 = __builtin_amdgcn_readlane(blk, s);                 // hyp[d - 1]: row d of lane 0
      const int xr = __builtin_amdgcn_update_dpp(0, xprev, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
      const int recv = __builtin_amdgcn_update_dpp(0, vlast, 0x138, 0xf, 0xf, false);
      const int x = L == 0 ? x0 : xr;
      const int left = L == 0 ? i : recv, diag = L == 0 ? i - 1 : left_prev;
      int nv[NC];
      {
        const int dg = diag + (x != lab[0] ? 1 : 0), de = left + 1, in = up[0] + 1;
        nv[0] = min(min(dg, de), in);
        mv[0] |= (dg == nv[0] ? 0u : de == nv[0] ? 1u : 2u) << (2 * (d & 15));
      }
#pragma unroll
      for (int c = 1; c < NC; ++c) {
        const int dg = up[c - 1] + (x != lab[c] ? 1 : 0), de = nv[c - 1] + 1, in = up[c] + 1;
        nv[c] = min(min(dg, de), in);
        mv[c] |= (dg == nv[c] ? 0u : de == nv[c] ? 1u : 2u) << (2 * (d & 15));
      }
      if (active) {
#pragma unroll
        for (int c = 0; c < NC; ++c) up[c] = nv[c];
        vlast = nv[NC - 1];
        left_prev = recv;
      }
      xprev = x;
      if ((d & 15) == 15 || d == steps) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          moves[((size_t)(d >> 4) * NC + c) * 64 + L] = mv[c];
          mv[c] = 0u;
        }
      }
    }
    blk = nxt;
  }
  if constexpr (!IN_LDS) __threadfence();
  __syncthreads();

#ifdef CTCN_EDIT_OPS_FORWARD_ONLY   // measurement builds (tools/edit_ops_bench.py --forward-only): stop before the walk -- outputs are NOT valid
  if (L == 0) counts[(size_t)u * 6] = nh + nr;
  return;
#endif
  // ---- 3. the walk back ------------------------------------------------------------------------------------------------------------
  const int cap = lda + ldb;
  int32_t *row = ali ? ali + (size_t)u * cap * 2 : nullptr;
  int n = 0;
  if (L == 0) {
    int i = nh, j = nr, n_sub = 0, n_del = 0, n_ins = 0, n_cor = 0;
    while (i > 0 || j > 0) {
      // the move word and both symbols are fetched together (their addresses depend on (i, j) alone): one memory round trip per pair
      const int jj = max(j - 1, 0), ii = max(i - 1, 0);
      const int lane = jj / NC, c = jj % NC, d = i + lane;
      const uint32_t word = moves[((size_t)(d >> 4) * NC + c) * 64 + lane];
      const int rj = ref[jj], hi = hyp[ii];
      const int m = i == 0 ? 1 : j == 0 ? 2 : (int)((word >> (2 * (d & 15))) & 3u);
      const int r = m != 2 ? rj : -1, h = m != 1 ? hi : -1;
      j -= m != 2;
      i -= m != 1;
      if (m == 0) { if (r == h) ++n_cor; else ++n_sub; }
      else if (m == 1) ++n_del;
      else ++n_ins;
      if (row) {
        row[2 * (size_t)(cap - 1 - n)] = r;
        row[2 * (size_t)(cap - 1 - n) + 1] = h;
      }
      if (conf) {
        const bool r_in = r >= 0 && r < V, h_in = h >= 0 && h < V;
        if ((m == 0 && r_in && h_in) || (m == 1 && r_in) || (m == 2 && h_in))
          atomicAdd(&conf[(size_t)(m == 2 ? V : r) * (V + 1) + (m == 1 ? V : h)], 1ull);
      }
      ++n;
    }
    int32_t *o = counts + (size_t)u * 6;
    o[0] = n_sub; o[1] = n_del; o[2] = n_ins; o[3] = n_cor; o[4] = nh; o[5] = nr;
    if (ali_len) ali_len[u] = n;
  }
  if (row == nullptr) return;
  n = __builtin_amdgcn_readfirstlane(n);
  __threadfence();
  __syncthreads();
  const int from = cap - n;
  for (int t0 = 0; t0 < cap; t0 += 64) {
    const int t = t0 + L;
    int r = -1, h = -1;
    if (t < n) { r = row[2 * (size_t)(from + t)]; h = row[2 * (size_t)(from + t) + 1]; }
    __syncthreads();                                    // every lane has its pair before any lane overwrites one (from may be < 64)
    if (t < cap) { row[2 * (size_t)t] = r; row[2 * (size_t)t + 1] = h; }
  }
}

}  // namespace

extern "C" size_t ctcn_edit_ops_ws_bytes(int B, int lda, int max_b_len) {
  if (B <= 0 || lda < 0 || max_b_len < 0 || max_b_len > 512 || edit_ops_in_lds(lda, max_b_len)) return 0;
  return (size_t)B * (edit_ops_hyp_words(lda) + edit_ops_move_words(lda, max_b_len)) * sizeof(uint32_t);
}

extern "C" int ctcn_edit_ops(const int32_t *a, const int32_t *a_len, const int64_t *b, const int64_t *b_len, const int32_t *map, int V,
                             int32_t *counts, int32_t *ali, int32_t *ali_len, long long *conf, int B, int lda, int ldb, int max_b_len,
                             void *ws, size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(a && a_len && b_len && counts && (b || ldb == 0) && B > 0 && lda >= 0 && ldb >= 0 && max_b_len >= 0, "ctcn_edit_ops: bad args");
  CTCN_REQUIRE(V >= 0 && ((!map && !conf) || V > 0), "ctcn_edit_ops: a class map or a confusion table needs V > 0 (V %d)", V);
  CTCN_REQUIRE((size_t)lda + (size_t)ldb < (1u << 30), "ctcn_edit_ops: lda + ldb too large");
  if (max_b_len > 512) { ctcn_set_error("ctcn_edit_ops: label length %d > 512 unsupported", max_b_len); return CTCN_EUNSUPPORTED; }
  const bool in_lds = edit_ops_in_lds(lda, max_b_len);
  const size_t need = ctcn_edit_ops_ws_bytes(B, lda, max_b_len);
  if (!in_lds) {
    CTCN_REQUIRE(ws && ((uintptr_t)ws & 3) == 0, "ctcn_edit_ops: workspace of ctcn_edit_ops_ws_bytes needed (lda %d, max_b_len %d), 4-byte aligned", lda, max_b_len);
    if (ws_bytes < need) { ctcn_set_error("ctcn_edit_ops: workspace %zu < %zu bytes", ws_bytes, need); return CTCN_EWORKSPACE; }
  }
  const int ref_words = (int)edit_ops_ref_words(max_b_len), hyp_words = (int)edit_ops_hyp_words(lda);
  const size_t ws_words = edit_ops_hyp_words(lda) + edit_ops_move_words(lda, max_b_len);
  const size_t sm = (in_lds ? ref_words + ws_words : (size_t)ref_words) * sizeof(uint32_t);
  hipStream_t st = (hipStream_t)stream;
  const int nc = edit_ops_nc(max_b_len);
#define EDIT_OPS_LAUNCH(NC, LDS) hipLaunchKernelGGL((edit_ops_wave_kernel<NC, LDS>), dim3(B), dim3(64), sm, st, a, a_len, b, b_len, map, V, counts, ali, ali_len, (unsigned long long *)conf, lda, ldb, max_b_len, (uint32_t *)ws, ws_words, ref_words, hyp_words)
  if (in_lds) {
    if (nc == 1) EDIT_OPS_LAUNCH(1, true); else if (nc == 2) EDIT_OPS_LAUNCH(2, true); else if (nc == 4) EDIT_OPS_LAUNCH(4, true); else EDIT_OPS_LAUNCH(8, true);
  } else {
    if (nc == 1) EDIT_OPS_LAUNCH(1, false); else if (nc == 2) EDIT_OPS_LAUNCH(2, false); else if (nc == 4) EDIT_OPS_LAUNCH(4, false); else EDIT_OPS_LAUNCH(8, false);
  }
#undef EDIT_OPS_LAUNCH
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
