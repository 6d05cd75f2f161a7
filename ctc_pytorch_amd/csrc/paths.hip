// paths.hip -- what is done with a per-frame class path or a token string once the network has answered: none of it is the CTC loss (ctc.hip).
//
// Kernels (contracts in include/ctcn.h):
//   greedy_collapse    : ctcn_greedy_collapse -- a wave per utterance drops repeats and blanks from the arg-max path (ballot + popcount).
//   path_tokens        : ctcn_path_tokens -- the tokens of a path with their frames, mean / min log-prob, margin and the path's score.
//   edit_distance      : ctcn_edit_distance -- Levenshtein distance of the collapsed prediction to the label, a lane per utterance with the DP
//   edit_distance_wave   row in LDS, or (option "edit_wave", labels up to 512) a wavefront per utterance along anti-diagonals.  The alignment
//                        behind a distance (operations, confusions) is ctcn_edit_ops, editops.hip.
//   step_stats         : ctcn_step_stats -- loss, distance sum, label-length sum and status word of a training step as four doubles.
#include <algorithm>

#include "common.h"

namespace {

__global__ void greedy_collapse_kernel(const int32_t *__restrict__ idx, size_t st_t, size_t st_b, const int32_t *__restrict__ lens,
                                       int32_t *__restrict__ out_ids, int32_t *__restrict__ out_len, int T, int B, int blank) {
  // one wave per utterance: 64 frames per iteration, ballot + popcount compaction (order preserving)
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= B) return;
  const int n = min(max(lens[b], 0), T);
  int base = 0;
  for (int t0 = 0; t0 < n; t0 += 64) {
    const int t = t0 + lane;
    int k = blank;
    bool keep = false;
    if (t < n) {
      k = idx[t * st_t + b * st_b];
      keep = k != blank && (t == 0 || k != idx[(t - 1) * st_t + b * st_b]);
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) out_ids[(size_t)b * T + base + __popcll(mask & ((1ull << lane) - 1ull))] = k;
    base += __popcll(mask);
  }
  if (lane == 0) out_len[b] = base;
}

// Tokens of a per-frame class path with their frames and scores (ctcn_path_tokens; the definition is in include/ctcn.h).  One workgroup
// per utterance, PT_THREADS frames per chunk, two phases per chunk:
//   A (all four waves): 16 lanes per frame gather lp[t, b, k] and, for a frame inside a token, max_{c != k} lp[t, b, c] (one pass over the
//     row, a 4-step butterfly), into LDS.  Blank frames read their one element, ids outside [0, V) nothing.
//   B (wave 0, 64 frames at a time): token starts by ballot (greedy_collapse_kernel's rule), the three per-token reductions by one segmented
//     inclusive scan (a start or a blank frame raises the flag that stops the scan), the token's first frame from the highest start bit at or
//     below the lane.  A run that is still open at lane 63 travels to the next 64 frames in wave-uniform carry registers and is added to the
//     lanes whose scan met no flag.  The lane that holds a run's last frame writes the token.
// -inf log-probs stay -inf in their own token only: nothing is a difference of prefix sums.
#define PT_THREADS 256
__device__ __forceinline__ int pt_class(const int32_t *__restrict__ path, size_t st_t, size_t st_b, int t, int b, int V) {
  const int k = path[(size_t)t * st_t + (size_t)b * st_b];
  return (k >= 0 && k < V) ? k : -1;
}
__global__ __launch_bounds__(PT_THREADS) void path_tokens_kernel(const int32_t *__restrict__ path, size_t st_t, size_t st_b, const float *__restrict__ lp,
                                                                 const int32_t *__restrict__ lens, int32_t *__restrict__ out_ids, int32_t *__restrict__ out_len,
                                                                 int32_t *__restrict__ starts, int32_t *__restrict__ ends, float *__restrict__ tok_mean,
                                                                 float *__restrict__ tok_min, float *__restrict__ tok_margin, float *__restrict__ path_score,
                                                                 int T, int B, int V, int blank) {
  __shared__ float sx[PT_THREADS], sc[PT_THREADS];
  __shared__ int sk[PT_THREADS];                            // the chunk's class ids (-1: outside [0, V)), so that phase B reads the path from LDS
  __shared__ int s_base;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(lens[b], 0), T);
  const int grp = tid >> 4, sub = tid & 15;
  int base = 0, c_start = 0;                                // wave 0: tokens started so far; the open run's first frame and partial reductions
  double c_sum = 0.0, c_msum = 0.0, total = 0.0;
  float c_min = INFINITY;
  for (int t0 = 0; t0 < n; t0 += PT_THREADS) {
    // ---- A
    for (int f = 0; f < PT_THREADS / 16; ++f) {
      const int slot = f * 16 + grp, t = t0 + slot;
      if (t >= n) continue;                                 // (uniform over the 16 lanes of a frame)
      const int k = pt_class(path, st_t, st_b, t, b, V);
      float x = 0.0f, m = -INFINITY;
      if (k >= 0) {
        const float *row = lp + ((size_t)t * B + b) * V;
        if (k == blank) {
          x = row[k];
        } else {
          for (int c = sub; c < V; c += 16) {
            const float v = row[c];
            if (c == k) x = v; else m = fmaxf(m, v);
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
          x = __shfl(x, k & 15, 16);
        }
      }
      if (sub == 0) { sx[slot] = x; sc[slot] = m; sk[slot] = k; }
    }
    __syncthreads();
    // ---- B
    if (wave == 0) {
      for (int s0 = 0; s0 < PT_THREADS && t0 + s0 < n; s0 += 64) {
        const int t = t0 + s0 + lane;
        const bool live = t < n;
        int kn = blank, kp = blank, kx = blank;
        float x = 0.0f, comp = 0.0f;
        if (live) {
          const int slot = s0 + lane;                       // (only the chunk's first and last frame look at the path itself)
          kn = sk[slot];
          if (t > 0) kp = slot > 0 ? sk[slot - 1] : pt_class(path, st_t, st_b, t - 1, b, V);
          if (t + 1 < n) kx = slot + 1 < PT_THREADS ? sk[slot + 1] : pt_class(path, st_t, st_b, t + 1, b, V);
          kn = kn < 0 ? blank : kn; kp = kp < 0 ? blank : kp; kx = kx < 0 ? blank : kx;
          x = sx[slot];
          comp = sc[slot];
        }
        total += (double)x;
        const bool member = live && kn != blank;
        const bool head = member && (t == 0 || kn != kp);
        const bool last = member && (t + 1 >= n || kx != kn);
        double sum = member ? (double)x : 0.0, msum = member ? (double)x - (double)comp : 0.0;
        float mn = member ? x : INFINITY;
        int flag = (head || !member) ? 1 : 0;
        for (int o = 1; o < 64; o <<= 1) {
          const double s2 = __shfl_up(sum, o, 64), m2 = __shfl_up(msum, o, 64);
          const float n2 = __shfl_up(mn, o, 64);
          const int f2 = __shfl_up(flag, o, 64);
          if (lane >= o && !flag) { sum += s2; msum += m2; mn = fminf(mn, n2); flag = f2; }
        }
        const unsigned long long heads = __ballot(head);
        const unsigned long long le = heads & ((2ull << lane) - 1ull);
        int start = le ? t0 + s0 + 63 - __clzll(le) : c_start;
        if (!flag) { sum += c_sum; msum += c_msum; mn = fminf(mn, c_min); }      // no start and no blank at or below this lane: the carried run
        if (last) {
          const size_t j = (size_t)b * T + (base + __popcll(le) - 1);
          const double cnt = (double)(t + 1 - start);
          out_ids[j] = kn; starts[j] = start; ends[j] = t + 1;
          tok_mean[j] = (float)(sum / cnt); tok_min[j] = mn; tok_margin[j] = (float)(msum / cnt);
        }
        base += __popcll(heads);
        c_sum = __shfl(sum, 63, 64); c_msum = __shfl(msum, 63, 64); c_min = __shfl(mn, 63, 64); c_start = __shfl(start, 63, 64);
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    if (lane == 0) { s_base = base; out_len[b] = base; path_score[b] = (float)total; }
  }
  __syncthreads();
  for (int j = s_base + tid; j < T; j += PT_THREADS) {
    const size_t o = (size_t)b * T + j;
    out_ids[o] = -1; starts[o] = -1; ends[o] = -1;
    tok_mean[o] = 0.0f; tok_min[o] = 0.0f; tok_margin[o] = 0.0f;
  }
}

// Levenshtein distance between the collapsed prediction a[b,:a_len[b]] (int32) and the label b[b,:b_len[b]] (int64):
// one lane per utterance, DP row in LDS (row stride ldrow), sequential over the O(La*Lb) cells of its utterance.
__global__ void edit_distance_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ a_len, const int64_t *__restrict__ bl,
                                     const int64_t *__restrict__ b_len, int32_t *__restrict__ out, int B, int lda, int ldb, int ldrow) {
  extern __shared__ int rows[];
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= B) return;
  int *row = rows + (size_t)threadIdx.x * ldrow;
  const int la = min(max(a_len[u], 0), lda), lb = (int)min(max(b_len[u], (int64_t)0), (int64_t)min(ldrow - 2, ldb));   // never beyond the row / the buffers
  const int32_t *pa = a + (size_t)u * lda;
  const int64_t *pb = bl + (size_t)u * ldb;
  for (int j = 0; j <= lb; ++j) row[j] = j;
  for (int i = 1; i <= la; ++i) {
    int diag = row[0];
    row[0] = i;
    const int x = pa[i - 1];
    for (int j = 1; j <= lb; ++j) {
      const int up = row[j];
      const int v = min(min(up + 1, row[j - 1] + 1), diag + (x != (int)pb[j - 1]));
      diag = up;
      row[j] = v;
    }
  }
  out[u] = row[lb];
}

// The same distance on one wavefront per utterance, along anti-diagonals: lane L owns the NC label columns L*NC+1 .. (L+1)*NC and
// at step d fills row i = d - L of them, so the only cross-lane traffic per step is one DPP shift (the right-most cell of the
// left neighbour, which that lane finished one step earlier; its value of two steps ago is the diagonal).  la + 63 steps of ~5
// dependent instructions instead of la*lb sequential LDS round trips: 1 230 -> ~25 us for 32 x (800 x 50) (tools/epoch_probe.py).
template <int NC>
__global__ __launch_bounds__(64) void edit_distance_wave_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ a_len, const int64_t *__restrict__ bl,
                                                                const int64_t *__restrict__ b_len, int32_t *__restrict__ out, int lda, int ldb, int max_b_len) {
  extern __shared__ int pred[];
  const int u = blockIdx.x, L = threadIdx.x;
  const int la = min(max(a_len[u], 0), lda), lb = (int)min(max(b_len[u], (int64_t)0), (int64_t)min(max_b_len, ldb));
  const int32_t *pa = a + (size_t)u * lda;
  const int64_t *pb = bl + (size_t)u * ldb;
  for (int i = L; i < la; i += 64) pred[i] = pa[i];
  int lab[NC], up[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = L * NC + c + 1;
    lab[c] = j <= lb ? (int)pb[j - 1] : -1;
    up[c] = j;                                          // row 0
  }
  int vlast = (L + 1) * NC, left_prev = L * NC;
  __syncthreads();
  int x = (L == 0 && la > 0) ? pred[0] : 0;             // prediction symbol of the row this lane fills at step 1
  for (int d = 1; d <= la + 63; ++d) {
    const int i = d - L;
    const bool active = i >= 1 && i <= la;
    const int xn = (i >= 0 && i < la) ? pred[i] : 0;    // next step's symbol (row i + 1), fetched off the dependent chain
    const int recv = __builtin_amdgcn_update_dpp(0, vlast, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const int left = L == 0 ? i : recv, diag = L == 0 ? i - 1 : left_prev;
    int nv[NC];
    nv[0] = min(min(up[0] + 1, left + 1), diag + (x != lab[0] ? 1 : 0));
#pragma unroll
    for (int c = 1; c < NC; ++c) nv[c] = min(min(up[c] + 1, nv[c - 1] + 1), up[c - 1] + (x != lab[c] ? 1 : 0));
    if (active) {
#pragma unroll
      for (int c = 0; c < NC; ++c) up[c] = nv[c];
      vlast = nv[NC - 1];
      left_prev = recv;
    }
    x = xn;
  }
  if (lb == 0) {
    if (L == 0) out[u] = la;
  } else if (L == (lb - 1) / NC) {
    const int cc = (lb - 1) % NC;
    int r = up[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) r = c == cc ? up[c] : r;
    out[u] = r;
  }
}

}  // namespace

// (loss, sum of the edit distances, sum of the label lengths, status word) of a training step as four doubles: what
// steps/train_ctc.run_epoch copies to the host one step behind -- one launch instead of nine small torch kernels
__global__ void step_stats_kernel(const float *__restrict__ loss, const int32_t *__restrict__ dist, const int64_t *__restrict__ tgt_len, int B,
                                  const int32_t *__restrict__ status, double *__restrict__ out) {
  const int lane = threadIdx.x;
  long long d = 0, n = 0;
  for (int b = lane; b < B; b += 64) { d += dist[b]; n += tgt_len[b]; }
  for (int o = 32; o > 0; o >>= 1) { d += __shfl_down(d, o, 64); n += __shfl_down(n, o, 64); }
  if (lane == 0) {
    out[0] = (double)loss[0];
    out[1] = (double)d;
    out[2] = (double)n;
    out[3] = status ? (double)status[0] : 0.0;
  }
}

extern "C" int ctcn_greedy_collapse(const int32_t *idx, size_t stride_t, size_t stride_b, const int32_t *lens, int32_t *out_ids,
                                    int32_t *out_len, int T, int B, int blank, void *stream) {
  CTCN_REQUIRE(idx && lens && out_ids && out_len && T > 0 && B > 0, "ctcn_greedy_collapse: bad args");
  hipLaunchKernelGGL(greedy_collapse_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, (hipStream_t)stream, idx, stride_t, stride_b, lens, out_ids, out_len, T, B, blank);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_path_tokens(const int32_t *path, size_t stride_t, size_t stride_b, const float *lp, const int32_t *lens, int32_t *out_ids,
                                int32_t *out_len, int32_t *starts, int32_t *ends, float *tok_mean, float *tok_min, float *tok_margin,
                                float *path_score, int T, int B, int V, int blank, void *stream) {
  CTCN_REQUIRE(path && lp && lens && out_ids && out_len && starts && ends && tok_mean && tok_min && tok_margin && path_score, "ctcn_path_tokens: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0, "ctcn_path_tokens: bad dims");
  CTCN_REQUIRE(blank >= 0 && blank < V, "ctcn_path_tokens: blank %d outside [0, %d)", blank, V);
  hipLaunchKernelGGL(path_tokens_kernel, dim3(B), dim3(PT_THREADS), 0, (hipStream_t)stream, path, stride_t, stride_b, lp, lens, out_ids, out_len, starts,
                     ends, tok_mean, tok_min, tok_margin, path_score, T, B, V, blank);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_edit_distance(const int32_t *a, const int32_t *a_len, const int64_t *b, const int64_t *b_len, int32_t *out,
                                  int B, int lda, int ldb, int max_b_len, void *stream) {
  CTCN_REQUIRE(a && a_len && b_len && out && (b || ldb == 0) && B > 0 && max_b_len >= 0, "ctcn_edit_distance: bad args");
  if (max_b_len <= 512 && (size_t)lda * sizeof(int) <= 60 * 1024 && ctcn_get_option("edit_wave") != 0) {
    const size_t sm = (size_t)std::max(lda, 1) * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    if (max_b_len <= 64) hipLaunchKernelGGL(edit_distance_wave_kernel<1>, dim3(B), dim3(64), sm, st, a, a_len, b, b_len, out, lda, ldb, max_b_len);
    else if (max_b_len <= 128) hipLaunchKernelGGL(edit_distance_wave_kernel<2>, dim3(B), dim3(64), sm, st, a, a_len, b, b_len, out, lda, ldb, max_b_len);
    else if (max_b_len <= 256) hipLaunchKernelGGL(edit_distance_wave_kernel<4>, dim3(B), dim3(64), sm, st, a, a_len, b, b_len, out, lda, ldb, max_b_len);
    else hipLaunchKernelGGL(edit_distance_wave_kernel<8>, dim3(B), dim3(64), sm, st, a, a_len, b, b_len, out, lda, ldb, max_b_len);
    CTCN_LAUNCH_CHECK();
    return CTCN_OK;
  }
  const int ldrow = max_b_len + 2;
  int threads = 64;
  while (threads > 1 && (size_t)threads * ldrow * sizeof(int) > 48 * 1024) threads >>= 1;
  if ((size_t)threads * ldrow * sizeof(int) > 48 * 1024) { ctcn_set_error("ctcn_edit_distance: label length %d too long", max_b_len); return CTCN_EUNSUPPORTED; }
  hipLaunchKernelGGL(edit_distance_kernel, dim3(ceil_div(B, threads)), dim3(threads), (size_t)threads * ldrow * sizeof(int),
                     (hipStream_t)stream, a, a_len, b, b_len, out, B, lda, ldb, ldrow);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_step_stats(const float *loss, const int32_t *dist, const int64_t *tgt_len, int B, const int32_t *status, double *out4,
                               void *stream) {
  CTCN_REQUIRE(loss && dist && tgt_len && out4 && B > 0, "ctcn_step_stats: bad args");
  hipLaunchKernelGGL(step_stats_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, dist, tgt_len, B, status, out4);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
