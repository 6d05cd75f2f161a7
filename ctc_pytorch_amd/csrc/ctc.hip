// ctc.hip -- log_softmax (+arg-max) and the CTC loss for gfx950: target packing, alpha/beta lattices, gradient, forced alignment.
// (What is done with a path or a token string afterwards -- greedy collapse, path tokens, edit distance, step statistics -- is paths.hip.)
//
// replaces: nn.LogSoftmax(dim=-1) (reference timit/models/model_ctc.py:140,168,181), torch.max(out,-1)
// (timit/steps/train_ctc.py:51, timit/utils/ctcDecoder.py:163) and nn.CTCLoss forward + autograd backward
// (train_ctc.py:144,47-48,63).  Arithmetic: SURVEY Appendix A.6-A.8.  torch's whole nn.CTCLoss contract: any blank index (a
// run-time argument: the lattice's skip rule is a parity test on the state, not a comparison with the blank's value), the
// reductions 'none' / 'sum' / 'mean' (the gradient scale of utterance b is gscale[b * stride], times 1 / (B * max(L_b, 1)) for
// 'mean'; the reductions themselves are ctcn_ctc_reduce, elementwise.hip) and zero_infinity (an infeasible utterance gives
// nll = +inf; its gradient rows are NaN as in torch, or exact zeros with zero_infinity).  Concatenated 1-D targets are packed
// into the padded (B, Lmax) layout the lattice reads by ctc_pack_targets_kernel.
//
// Kernels (all HBM/latency-bound, no MFMA):
//   log_softmax fwd : one wave per row, lanes over classes, max / sum-exp by wave shuffles; the arg-max
//                     (lowest index on ties) is taken on the produced log-probs in the same pass.
//   ctc_alpha/beta  : one workgroup per utterance.  Lattices of up to 256 states (labels up to 127 symbols) run wave-skewed
//                     (ctc_lattices_skew_kernel): one state per lane, the row in a register, neighbour states s-1, s-2
//                     by DPP wave shifts, the waves a pipeline that hands its edge states on through a small LDS ring
//                     once per 4-frame chunk -- no LDS trip and no barrier on a frame's chain (0.107 us per frame).
//                     Longer labels, the in-place beta pass and option "ctc_lattice_skew" = 0 take the classic kernels:
//                     the states live across 256 threads, alpha_{t-1} / beta_{t+1} in a double-buffered LDS row
//                     (neighbour states are LDS reads), one barrier per frame (0.233 us per frame).  Either way the
//                     log-prob gathers lp[t, ext(s)] are issued 4 frames ahead and the lattice stores never waited for.
//                     alpha is stored (T,B,S) for the backward, beta beside it (or folded into it: alpha+beta).
//   ctc_grad        : fully parallel over (t,b): one wave per frame; blank occupancy by a wave-wide
//                     log-sum-exp over the even states, label occupancy by a per-class scan of the label
//                     string (deterministic: fixed order, no atomics).
//   ctc_pack_targets: concatenated 1-D targets -> the padded (B, Lmax) rows the lattices read.
//   ctc_align       : forced alignment: the classic alpha walk in the max-plus semiring plus a back-pointer trace.
// Then, on the host, the two launch plans (lattice passes, alignment) and the extern "C" entry points in one block at the end.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace {

constexpr int CTC_THREADS = 256;
constexpr int CTC_NS = 16;  // lattice states per thread -> S <= 4096 (L <= 2047; 3 S floats of LDS = 48 KB)

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

template <bool WRITE_LP>
__global__ __launch_bounds__(256) void log_softmax_kernel(const float *__restrict__ in, float *__restrict__ lp,
                                                          int32_t *__restrict__ amax, int rows, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *x = in + (size_t)row * V;
  float m = -INFINITY;
  for (int c = lane; c < V; c += 64) m = fmaxf(m, x[c]);
  m = wave_max(m);
  float lse = 0.0f;
  if (WRITE_LP) {
    float s = 0.0f;
    for (int c = lane; c < V; c += 64) s += expf(x[c] - m);
    s = wave_sum(s);
    lse = m + logf(s);
  }
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < V; c += 64) {
    const float v = WRITE_LP ? x[c] - lse : x[c];
    if (WRITE_LP) lp[(size_t)row * V + c] = v;
    if (better(v, c, bv, bi)) { bv = v; bi = c; }
  }
  if (amax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) amax[row] = bi;
  }
}

__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(const float *__restrict__ lp, const float *__restrict__ dlp,
                                                              float *__restrict__ dx, int rows, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *l = lp + (size_t)row * V, *g = dlp + (size_t)row * V;
  float s = 0.0f;
  for (int c = lane; c < V; c += 64) s += g[c];
  s = wave_sum(s);
  for (int c = lane; c < V; c += 64) dx[(size_t)row * V + c] = g[c] - expf(l[c]) * s;
}

// log(e^x0 + e^x1 + e^x2) on the hardware exp2 / log2 (1 ulp each): the lattice recursion is a chain of T dependent
// steps per utterance, so the ~100 instructions of three expf + logf per step were most of its run time.  The sum is in
// [1, 3], so the log2 result carries an absolute error below 2e-7 per step.  All three -inf: -inf, as a select on the result and not a
// branch around the arithmetic -- the skewed loop has no branch and no exec change, and the classic loop is shorter without one per state.
__device__ __forceinline__ float lse3(float x0, float x1, float x2) {
  const float m = fmaxf(x0, fmaxf(x1, x2));
  const float L2E = 1.4426950408889634f;
  const float sum = __builtin_amdgcn_exp2f((x0 - m) * L2E) + __builtin_amdgcn_exp2f((x1 - m) * L2E) + __builtin_amdgcn_exp2f((x2 - m) * L2E);
  const float r = m + __builtin_amdgcn_logf(sum) * 0.6931471805599453f;
  return m == -INFINITY ? -INFINITY : r;
}

// ---- The length contract and the nll finish of every CTC kernel ----
// in_len[b] and tgt_len[b], read once.  bad: lengths a caller must not pass (torch.nn.CTCLoss raises) -- nothing of the lattice is defined: NaN
// loss, NaN gradient rows, no alignment; Tb, L and S then mean nothing (the kernels that go on with such an utterance, to fill its rows, take
// them as 0).  Otherwise Tb frames, L labels and S = 2 L + 1 lattice states.  (ctc_lattice_skew_body spells the same rule out: see there.)
struct CtcLens {
  int64_t in, tgt;
  int T, Lmax, Tb, L, S;
  __device__ __forceinline__ CtcLens(const int64_t *__restrict__ in_len, const int64_t *__restrict__ tgt_len, int b, int T_, int Lmax_)
      : in(in_len[b]), tgt(tgt_len[b]), T(T_), Lmax(Lmax_), Tb((int)in), L((int)tgt), S(2 * L + 1) {}
  __device__ __forceinline__ bool bad() const { return in < 0 || in > T || tgt < 0 || tgt > Lmax; }
};

// nll from the two final alpha states (l2 = -inf where the lattice has one state)
__device__ __forceinline__ float ctc_nll_from_final(float l1, float l2) {
  const float m = fmaxf(l1, l2);
  return m == -INFINITY ? INFINITY : -(m + logf(expf(l1 - m) + expf(l2 - m)));
}

// ---- The classic lattice walk (ctc_lattice_kernel, ctc_lattices_kernel, ctc_align_kernel's forward chain) ----
// One workgroup of CTC_THREADS per utterance, state s = tid + k * CTC_THREADS for k < NS (the host picks the smallest of 1/2/4/8/16 that covers
// Smax), the row of the frame before in a double-buffered LDS row (smem: two rows of Smax floats, then the ext[] row of Smax ints).
// DIR: +1 walks t = 0 .. Tb - 1 with neighbours s - 1, s - 2 (alpha), -1 walks t = Tb - 1 .. 0 with s + 1, s + 2 (beta).
// The recursion is a chain of Tb dependent steps whose per-step work is three LDS reads, one combine and one LDS write, so everything else is
// kept off that chain: the gathered log-probs (and whatever else the policy wants of a frame, Policy::prefetch) are fetched PF frames ahead into
// registers, the barrier between steps waits for LDS only, and what the policy stores to memory is never waited for.
// What differs between the users is the Policy -- the semiring and what a frame leaves behind:
//   float prefetch(t, s)                    a second value fetched with the gather of (t, s) and handed back to emit as `pre` (0.0f: none)
//   void  first(t, s, v)                    the first frame's value of state s < S
//   float combine(x0, x1, x2, q, int &tag)  the value of a state from prev[s], prev[s -/+ 1], prev[s -/+ 2] (-inf where the move does not exist)
//                                           and the gathered log-prob q; tag (0 on entry) is a by-product that emit gets back
//   void  emit(t, s, live, v, tag, pre)     called by EVERY lane, live = s < S (v and tag are 0 otherwise), so that it may hold wave-wide operations
// Returns the row of the last frame; only a barrier's worth of LDS ordering stands behind it (the walk's last lds_barrier, or the
// __syncthreads after the first frame when Tb == 1).  The caller has ruled out Tb <= 0.
template <int DIR, int NS, class Policy>
__device__ __forceinline__ const float *ctc_classic_walk(float *smem, const float *__restrict__ lp, const int64_t *__restrict__ targets, int Tb,
                                                         int S, int B, int V, int Lmax, int blank, const Policy &pol) {
  constexpr int PF = 4;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Smax = 2 * Lmax + 1;
  float *buf0 = smem, *buf1 = smem + Smax;
  int *ext = reinterpret_cast<int *>(smem + 2 * Smax);
  for (int s = tid; s < S; s += CTC_THREADS) ext[s] = (s & 1) ? (int)targets[(size_t)b * Lmax + (s >> 1)] : blank;
  __syncthreads();
  // per-thread static state info
  int my_ext[NS];
  bool my_skip[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * CTC_THREADS;
    my_ext[k] = 0; my_skip[k] = false;
    if (s < S) {
      my_ext[k] = ext[s];
      // label states (odd s) skip over the blank between two different labels; a label may equal any class value, the blank's included
      if (DIR > 0) my_skip[k] = s >= 2 && (s & 1) && ext[s] != ext[s - 2];
      else my_skip[k] = s + 2 < S && (s & 1) && ext[s] != ext[s + 2];
    }
  }
  const int t_first = DIR > 0 ? 0 : Tb - 1;
  // frame t_first
  {
    const float *lpt = lp + ((size_t)t_first * B + b) * V;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * CTC_THREADS;
      if (s < S) {
        float v = -INFINITY;
        if (DIR > 0) { if (s <= 1) v = lpt[my_ext[k]]; }
        else { if (s >= S - 2) v = lpt[my_ext[k]]; }
        buf0[s] = v;
        pol.first(t_first, s, v);
      }
    }
  }
  __syncthreads();
  float *prev = buf0, *cur = buf1;
  // frame n of the walk (the last one again past it: those loads are not used) into one slot of the prefetch ring
  auto fetch = [&](int n, float (&q)[NS], float (&a)[NS]) {
    const int t = t_first + DIR * min(n, Tb - 1);
    const float *lpt = lp + ((size_t)t * B + b) * V;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * CTC_THREADS;
      q[k] = s < S ? lpt[my_ext[k]] : 0.0f;
      a[k] = s < S ? pol.prefetch(t, s) : 0.0f;
    }
  };
  float nq[PF][NS], na[PF][NS];      // prefetched frames n0 .. n0+PF-1 of the NEXT chunk: log-prob gather / the policy's own value
#pragma unroll
  for (int i = 0; i < PF; ++i) fetch(1 + i, nq[i], na[i]);
  for (int n0 = 1; n0 < Tb; n0 += PF) {
    float cq[PF][NS], ca[PF][NS];
#pragma unroll
    for (int i = 0; i < PF; ++i)
#pragma unroll
      for (int k = 0; k < NS; ++k) { cq[i][k] = nq[i][k]; ca[i][k] = na[i][k]; }
    if (n0 + PF < Tb) {
#pragma unroll
      for (int i = 0; i < PF; ++i) fetch(n0 + PF + i, nq[i], na[i]);
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int n = n0 + i;
      if (n < Tb) {
        const int t = t_first + DIR * n;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const int s = tid + k * CTC_THREADS;
          float v = 0.0f;
          int tag = 0;
          if (s < S) {
            const float x0 = prev[s];
            float x1, x2;
            if (DIR > 0) { x1 = s >= 1 ? prev[s - 1] : -INFINITY; x2 = my_skip[k] ? prev[s - 2] : -INFINITY; }
            else { x1 = s + 1 < S ? prev[s + 1] : -INFINITY; x2 = my_skip[k] ? prev[s + 2] : -INFINITY; }
            v = pol.combine(x0, x1, x2, cq[i][k], tag);
            cur[s] = v;
          }
          pol.emit(t, s, s < S, v, tag, ca[i][k]);
        }
        lds_barrier();       // LDS only: the policy's stores and the prefetches stay in flight across timesteps
        float *tmp = prev; prev = cur; cur = tmp;
      }
    }
  }
  return prev;
}

// The sum semiring: alpha (DIR +1) and beta (DIR -1) into the lattice `lat` (T, B, Smax).  ACC (the beta pass of ctcn_ctc_bwd): every value is
// added to what `lat` holds -- alpha + beta in place, the one-buffer reserve; the old values are the policy's prefetched stream.  Otherwise the pass
// writes its own lattice, which lets alpha and beta run side by side in one launch (ctcn_ctc_fwd_both).
template <bool ACC>
struct CtcSumPolicy {
  float *__restrict__ lat;
  int B, b, Smax;
  __device__ __forceinline__ float *at(int t, int s) const { return lat + ((size_t)t * B + b) * Smax + s; }
  __device__ __forceinline__ float prefetch(int t, int s) const { return ACC ? *at(t, s) : 0.0f; }
  __device__ __forceinline__ void first(int t, int s, float v) const { *at(t, s) = ACC ? *at(t, s) + v : v; }
  __device__ __forceinline__ float combine(float x0, float x1, float x2, float q, int &) const { return lse3(x0, x1, x2) + q; }
  __device__ __forceinline__ void emit(int t, int s, bool live, float v, int, float pre) const {
    if (live) *at(t, s) = ACC ? pre + v : v;
  }
};

template <int DIR, int NS, bool ACC>
__device__ __forceinline__ void ctc_lattice_body(float *smem, const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                 const int64_t *__restrict__ in_len, const int64_t *__restrict__ tgt_len,
                                                 float *__restrict__ lat, float *__restrict__ nll, int T, int B, int V, int Lmax, int blank) {
  static_assert(!ACC || DIR < 0, "only the beta pass adds into the lattice it finds");
  const int b = blockIdx.x;
  const CtcLens len(in_len, tgt_len, b, T, Lmax);
  if (len.bad() || len.Tb <= 0) {          // no lattice to walk: the alpha pass answers nll -- NaN, 0 for the empty label on no frames, else +inf
    if (DIR > 0 && threadIdx.x == 0) nll[b] = len.bad() ? __uint_as_float(0x7fc00000u) : len.L == 0 ? 0.0f : INFINITY;
    return;                                // (before any barrier)
  }
  const CtcSumPolicy<ACC> pol{lat, B, b, 2 * Lmax + 1};
  const float *last = ctc_classic_walk<DIR, NS>(smem, lp, targets, len.Tb, len.S, B, V, Lmax, blank, pol);
  if (DIR > 0 && threadIdx.x == 0) nll[b] = ctc_nll_from_final(last[len.S - 1], len.S > 1 ? last[len.S - 2] : -INFINITY);
}

// one pass: alpha (DIR +1) into its own lattice, or beta (DIR -1) added into the alpha lattice in place (nll is not touched)
template <int DIR, int NS>
__global__ __launch_bounds__(CTC_THREADS) void ctc_lattice_kernel(const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                                  const int64_t *__restrict__ in_len,
                                                                  const int64_t *__restrict__ tgt_len, float *__restrict__ alpha,
                                                                  float *__restrict__ nll, int T, int B, int V, int Lmax, int blank) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  ctc_lattice_body<DIR, NS, (DIR < 0)>(smem, lp, targets, in_len, tgt_len, alpha, nll, T, B, V, Lmax, blank);
}

// alpha (blockIdx.y = 0) and beta (blockIdx.y = 1) of every utterance in one launch: the two passes are independent chains of
// T dependent steps, so running them side by side halves the latency of the loss (2B workgroups instead of B twice).
template <int NS>
__global__ __launch_bounds__(CTC_THREADS) void ctc_lattices_kernel(const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                                   const int64_t *__restrict__ in_len,
                                                                   const int64_t *__restrict__ tgt_len, float *__restrict__ alpha,
                                                                   float *__restrict__ beta, float *__restrict__ nll, int T, int B, int V,
                                                                   int Lmax, int blank) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (blockIdx.y == 0) ctc_lattice_body<1, NS, false>(smem, lp, targets, in_len, tgt_len, alpha, nll, T, B, V, Lmax, blank);
  else ctc_lattice_body<-1, NS, false>(smem, lp, targets, in_len, tgt_len, beta, nll, T, B, V, Lmax, blank);
}

// (Measured and dropped: one wave per (utterance, pass) with the lattice in registers -- lane l holding states 2l and 2l + 1,
// no LDS, no barrier -- is bit-identical but not faster at cfg2: neighbour states through ds_bpermute 230 us (round 1); through DPP
// wave shifts (one per alpha step), with hand-counted vmcnt for the gathers / lattice stores, pointer-stepped addressing and a
// two-term lse for the blank states: 195 us, the same as the 193-195 us of ctc_lattice_kernel (round 2).  With lse3 replaced by a max the
// wave version takes 101 us: a step is ~280 cycles of quarter-rate transcendentals (5 exp2 + 2 log2 per lane holding two states)
// + ~300 cycles of everything else, and neither is the exchange.)

// ---- The wave-skewed lattice (option "ctc_lattice_skew", plan_ctc_lattice) ----
// ONE state per lane, s = 64 w + lane, on Wl = ceil(Smax / 64) <= 4 waves (the workgroup is 64 Wl threads), the lattice row in a register:
// the arithmetic of a frame is the classic body's (lse3 of the same three operands in the same order, then + the gathered log-prob), so every
// stored value has the classic kernel's bits; what changes is where the neighbour states come from.
//   inside a wave   : s -/+ 1 is one DPP wave shift of the row register (wave_shr:1 for alpha, wave_shl:1 for beta), s -/+ 2 the shift applied
//                     to the shifted row.  The shifts run with all 64 lanes enabled (the frame loop is wave-uniform); states past the
//                     utterance's S, and the skip rule, are selects on the VALUES: a lane with s >= S adds 0 instead of a log-prob, so it
//                     holds -inf for ever, which is what the classic `s + 1 < S` test substitutes.
//   across waves    : alpha needs lower states only and beta higher ones, so the waves form a pipeline.  Frames 1 .. Tb - 1 (counted from the
//                     pass's first frame) go in chunks of CTC_CHUNK = 4, C = ceil((Tb - 1) / 4) of them; one loop trip is one chunk and ends in
//                     `s_waitcnt lgkmcnt(0); s_barrier`.  With Wb = ceil(S / 64) the waves that hold a state of THIS utterance, rank r = w (alpha)
//                     or Wb - 1 - w (beta), the wave of rank r computes chunk c in trip c + r K, K = CTC_SKEW = 3 trips behind its predecessor.
//                     The two edge values (lanes 63, 62 for alpha; 0, 1 for beta) of the four frames that chunk c STARTS from -- frames 4 c ..
//                     4 c + 3, kept in registers while the chunk runs -- go to the successor through LDS slot `ring[w][c % CTC_RING]`.
// Measured (profiles/ctc_lattice_ab.txt; cfg2's lattice, T = 800, B = 32, S <= 121, two waves; cycles at 2.4 GHz):
//   classic kernel                                   186 us  0.233 us = 560 cycles per frame
//   a trip (ring accesses + barrier) per FRAME, K = 2 161 us  0.202 us = 485 cycles; cfg4's four waves 361 us against the classic 292: the ring
//                                                    accesses were off the chain, but the barrier's arrive-and-release is on every wave's chain
//                                                    and grows with the waves that meet at it; + two exec toggles around the ring write and the store
//   a trip per CHUNK of four frames, K = 3 (built)    86 us  0.107 us = 257 cycles; cfg4 139 us (0.116 us per frame), cfg1 30 us against 64
// A frame of the built loop is 24 VALU instructions (13 on the dependent chain: 2 DPP moves, select, max3, sub, mul, exp2, 2 adds, log2, fma,
// select, add; the other two sub / mul / exp2 share the issue: 4 quarter-rate transcendentals), ~8 scalar instructions that step the two row
// pointers and their buffer resources, one buffer store and one buffer load, no branch, no exec change and no wait on anything issued in the
// same chunk; a chunk adds two 16-byte ring reads, one 16-byte ring write, the wait and the barrier.  The two things the per-frame variant
// taught: a store under `if (s < S)` is an exec toggle and a branch per frame AND makes the compiler's vmcnt count inexact across the loop (it
// then waits for the youngest lattice store before the next gather is used) -- the range check of a buffer resource that ends at S drops
// those lanes instead; and a prefetched register must be reloaded in place, never copied at the loop's end while its load is in flight.
// Hand-off rule (barrier and ring depth only -- no flags, no spins, nothing rests on which wave is faster).  Both ring accesses of a trip are
// issued at its START and complete at its barrier, so neither is waited for on the arithmetic chain:
//   write : rank r stores slot c at the start of the trip after chunk c, trip c + 1 + r K (its first drain trip after the last chunk).
//   read  : rank r + 1 loads slot c one trip before it computes chunk c, in trip c - 1 + (r + 1) K.
//   read after write : c - 1 + (r + 1) K >  c + 1 + r K                       <=>  K >= 3.
//   slot reuse       : slot c + CTC_RING is written in trip c + CTC_RING + 1 + r K, after the read's trip  <=>  CTC_RING >= K - 1.
// CTC_RING = 4 >= K - 1 = 2 (a power of two: the slot is `c & 3`).
// Barrier count: every wave of the workgroup executes NT = C + (Wb - 1) K loop barriers -- r K fill trips (the last one issues the first
// read), C chunk trips, (Wb - 1 - r) K drain trips; a wave w >= Wb holds no state and only arrives NT times -- plus, in the alpha pass, one
// __syncthreads before thread 0 reads the two final states for nll.  NT depends on in_len[b] and tgt_len[b] alone.
// Cells written: exactly the classic kernel's (t < in_len[b], s < 2 L_b + 1); the length checks are the classic ones and return before any barrier.
// Serves CTC_ALPHA and CTC_ALPHA_BETA.  CTC_BETA_INTO_ALPHA (ctcn_ctc_bwd's in-place reserve) stays on ctc_lattice_kernel: its prefetch of
// the old alpha values is a second register stream with no counterpart here, and no product path launches it.
// SLOW (option "ctc_slow_wave", a bit per wave; parity harness as "rnn_slow_items"): the named waves sleep CTC_SLOW_SLEEP x 64 cycles before
// their ring read and after their ring write in every trip; the product instantiation carries no code for it.
constexpr int CTC_CHUNK = 4, CTC_SKEW = 3, CTC_RING = 4, CTC_SKEW_WAVES = 4, CTC_SLOW_SLEEP = 32;

// lds_barrier() with the wait as an instruction the compiler's own s_waitcnt placement sees: behind an opaque asm wait it waits again, with
// lgkmcnt(0), at the first use of a ring value loaded a trip earlier -- and so for the ring accesses just issued, on the chain.
__device__ __forceinline__ void skew_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);                                // lgkmcnt(0) only (gfx9 encoding: vmcnt 63, expcnt 7)
  asm volatile("s_barrier" ::: "memory");
}

// the row register shifted by one state towards the pass's direction; the lane with no source in this wave (0 / 63) takes `edge`
template <int DIR>
__device__ __forceinline__ float wave_shift1(float edge, float v) {
  return __int_as_float(DIR > 0 ? __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false)
                                : __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}

template <int DIR, bool SLOW>
__device__ __forceinline__ void ctc_lattice_skew_body(float *smem, const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                      const int64_t *__restrict__ in_len, const int64_t *__restrict__ tgt_len,
                                                      float *__restrict__ out, float *__restrict__ nll, int T, int B, int V, int Lmax, int blank,
                                                      int slow_mask) {
  constexpr int PF = 4, K = CTC_SKEW;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);           // wave-uniform for the compiler too: the trip loops are scalar loops
  const int Smax = 2 * Lmax + 1;
  // The classic body's length rule (CtcLens) spelt out: through the struct the compiler lays the kernel's blocks out differently around the same
  // chunk loops, which measures 0.6 us per launch slower at cfg2 (86.5 against 85.9 us; profiles/ctc_refactor_checks.txt)
  const int Tb = (int)in_len[b], L = (int)tgt_len[b];
  if (in_len[b] < 0 || in_len[b] > T || tgt_len[b] < 0 || tgt_len[b] > Lmax) {
    if (DIR > 0 && tid == 0) nll[b] = __uint_as_float(0x7fc00000u);
    return;
  }
  if (Tb <= 0) {
    if (DIR > 0 && tid == 0) nll[b] = L == 0 ? 0.0f : INFINITY;
    return;
  }
  const int S = 2 * L + 1, Wb = (S + 63) >> 6;
  const int C = (Tb - 1 + PF - 1) / PF;                             // chunks of frames 1 .. Tb - 1
  const int NT = C + (Wb - 1) * K;
  float4 *ring = reinterpret_cast<float4 *>(smem);                  // [waves][CTC_RING][2]: edge 0 / edge 1 of a chunk's four start frames
  float *fin = smem + 8 * CTC_RING * (int)(blockDim.x >> 6);        // the two final alpha states
  if (w < Wb) {
    const int s = tid;
    const bool live = s < S;
    const bool slow = SLOW && ((slow_mask >> w) & 1);
    const int r = DIR > 0 ? w : Wb - 1 - w;
    const bool has_pred = r > 0;
    const int prow = (has_pred ? w - DIR : w) * CTC_RING;            // the predecessor's ring row (rank 0: its own, the value is dropped)
    const int edge = DIR > 0 ? 63 - lane : lane;                      // 0 / 1 in the two lanes whose states the successor reads
    // static state info straight from the label string (one state per lane: no ext[] row in LDS)
    const int64_t *tg = targets + (size_t)b * Lmax;
    unsigned my_ext = (unsigned)blank;                                // (as a byte offset below: 32-bit lane offsets on wave-uniform row pointers)
    bool my_skip = false;
    if (live && (s & 1)) {
      const int j = s >> 1;
      my_ext = (unsigned)(int)tg[j];
      if (DIR > 0) my_skip = s >= 2 && (int)tg[j] != (int)tg[j - 1];
      else my_skip = s + 2 < S && (int)tg[j] != (int)tg[j + 1];
    }
    const ptrdiff_t lp_step = (ptrdiff_t)DIR * B * V, out_step = (ptrdiff_t)DIR * B * Smax;
    const int t_first = DIR > 0 ? 0 : Tb - 1;
    const float *lpt = lp + ((size_t)t_first * B + b) * V;           // wave-uniform row pointers, stepped once per frame
    float *orow = out + ((size_t)t_first * B + b) * Smax;
    const unsigned ext_off = my_ext * 4u, s_off = (unsigned)s * 4u;
    // Rows through buffer resources built from the wave-uniform row pointer: no per-lane 64-bit address, and the lattice row's resource ends at
    // the utterance's S, so the store of a lane past it is dropped by the range check -- no branch (and no exec toggling) around the store, which
    // also keeps the compiler's vmcnt counting exact across the loop.  (A label outside [0, V) gathers 0.0 instead of reading past the row.)
    auto gather = [&](const float *row) {
      return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(row), 0, V * 4, 0x00020000), ext_off, 0, 0));
    };
    auto put = [&](float *row, float v) {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), __builtin_amdgcn_make_buffer_rsrc(row, 0, S * 4, 0x00020000), s_off, 0, 0);
    };
    float a = -INFINITY;                                             // the lattice row: this lane's state of the last frame done
    if (live && (DIR > 0 ? s <= 1 : s >= S - 2)) a = gather(lpt);
    put(orow, a);
    // log-prob gathers PF frames ahead; the pointer stops at the last frame (its extra loads are not used).  A lane past S loads the blank's
    // log-prob and adds 0 instead.
    float q[PF];                                                     // q[i]: frame n + i of the running chunk, reloaded in place for frame n + i + PF
    const float *lpn = lpt;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      if (1 + i < Tb) lpn += lp_step;
      q[i] = gather(lpn);
    }
    const float4 ninf4 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    auto ring_read = [&](int c, float4 &x, float4 &y) {
      if (slow) __builtin_amdgcn_s_sleep(CTC_SLOW_SLEEP);
      const float4 *slot = ring + 2 * (prow + (c & (CTC_RING - 1)));
      x = slot[0]; y = slot[1];
      if (!has_pred) { x = ninf4; y = ninf4; }
    };
    auto ring_write = [&](int c, const float (&h)[PF]) {
      if (edge <= 1) ring[2 * (w * CTC_RING + (c & (CTC_RING - 1))) + edge] = make_float4(h[0], h[1], h[2], h[3]);
      if (slow) __builtin_amdgcn_s_sleep(CTC_SLOW_SLEEP);
    };
    // fill: r K trips; the last one issues the read of the predecessor's slot 0
    float4 ex = ninf4, ey = ninf4;                                   // the predecessor's edges of this chunk's start frames
    for (int j = 0; j < r * K; ++j) {
      if (j == r * K - 1) ring_read(0, ex, ey);
      skew_barrier();
    }
    float hist[PF] = {a, a, a, a};                                   // this lane's state at the chunk's four start frames
    auto frame = [&](float e0, float e1, float q) {
      const float x1 = wave_shift1<DIR>(e0, a);
      const float x2r = wave_shift1<DIR>(e1, x1);
      const float v = lse3(a, x1, my_skip ? x2r : -INFINITY) + q;
      orow += out_step;
      put(orow, v);
      a = v;
    };
    // One chunk.  FAST: its four frames and the four it prefetches all exist -- no checks, plain pointer steps.  A log-prob register is
    // reloaded in place right after its frame (no copy of a register with a load in flight, which would be waited for with everything
    // younger, the lattice stores included); the select for lanes past S sits at the use, four frames after the load.
    auto chunk = [&](int c, auto fast) {
      constexpr bool FAST = decltype(fast)::value;
      // ring traffic first, off the chain: my edges of chunk c - 1's start frames, the predecessor's of chunk c + 1's
      float4 nx, ny;
      if (c > 0) ring_write(c - 1, hist);
      ring_read(c + 1, nx, ny);
      const int n = 1 + c * PF;
      const float e0[PF] = {ex.x, ex.y, ex.z, ex.w}, e1[PF] = {ey.x, ey.y, ey.z, ey.w};
#pragma unroll
      for (int i = 0; i < PF; ++i) {
        hist[i] = a;
        if (FAST || n + i < Tb) frame(e0[i], e1[i], live ? q[i] : 0.0f);
        if (FAST || n + i + PF < Tb) lpn += lp_step;
        q[i] = gather(lpn);
      }
      ex = nx; ey = ny;
      skew_barrier();
    };
    int c = 0;
    for (; 1 + c * PF + 2 * PF <= Tb; ++c) chunk(c, std::true_type());
    for (; c < C; ++c) chunk(c, std::false_type());
    if (DIR > 0) {
      if (s == S - 1) fin[0] = a;
      if (s == S - 2) fin[1] = a;
    }
    for (int j = 0; j < (Wb - 1 - r) * K; ++j) {
      if (j == 0 && C > 0) ring_write(C - 1, hist);
      skew_barrier();
    }
  } else {
    for (int j = 0; j < NT; ++j) skew_barrier();
  }
  if (DIR > 0) {
    __syncthreads();
    if (tid == 0) nll[b] = ctc_nll_from_final(fin[0], S > 1 ? fin[1] : -INFINITY);
  }
}

// grid (B) with beta == nullptr: alpha alone; grid (B, 2): alpha (y = 0) and beta (y = 1) side by side, as ctc_lattices_kernel
template <bool SLOW>
__global__ __launch_bounds__(64 * CTC_SKEW_WAVES) void ctc_lattices_skew_kernel(const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                                                const int64_t *__restrict__ in_len,
                                                                                const int64_t *__restrict__ tgt_len, float *__restrict__ alpha,
                                                                                float *__restrict__ beta, float *__restrict__ nll, int T, int B,
                                                                                int V, int Lmax, int blank, int slow_mask) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (blockIdx.y == 0) ctc_lattice_skew_body<1, SLOW>(smem, lp, targets, in_len, tgt_len, alpha, nll, T, B, V, Lmax, blank, slow_mask);
  else ctc_lattice_skew_body<-1, SLOW>(smem, lp, targets, in_len, tgt_len, beta, nll, T, B, V, Lmax, blank, slow_mask);
}

// online log-sum-exp accumulator
struct Lse {
  float m, s;
  __device__ __forceinline__ void add(float x) {
    if (x == -INFINITY) return;
    if (x > m) { s = s * expf(m - x) + 1.0f; m = x; }
    else s += expf(x - m);
  }
};

// SEP: alpha and beta are separate lattices (`ab` = alpha, `bt` = beta) and are added here -- the same single f32 add the
// in-place beta pass performs, so both reserves give bit-identical gradients.
// One workgroup = GRAD_TCH frames of ONE utterance (grid (ceil(T / GRAD_TCH), B), a wave per frame in turn).  The gradient of class c
// at a frame is exp(lp) - exp(logsumexp over the label positions j with target[j] == c of alpha+beta - ...): instead of every class
// lane scanning all L labels at every frame (O(V L) per frame: 81 us at cfg2), the workgroup sorts the label positions by class once
// (counting sort in LDS, positions of a class in increasing order) and a class lane walks its own positions only -- the same terms
// added in the same order, so the result is bit-identical to the scan.
// Upstream gradient of utterance b: gscale[b * gs_stride] (stride 0: the scalar of 'sum' / 'mean', 1: the (B,) vector of 'none'), divided
// by B * max(L_b, 1) for 'mean'.  zinf (zero_infinity): the rows of an utterance with nll = +inf are exact zeros.
constexpr int GRAD_TCH = 16;
template <bool SEP>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                       const int64_t *__restrict__ in_len, const int64_t *__restrict__ tgt_len,
                                                       const float *__restrict__ ab, const float *__restrict__ bt,
                                                       const float *__restrict__ nll,
                                                       const float *__restrict__ gscale, int gs_stride, int mean, int zinf, int blank,
                                                       float *__restrict__ grad, int T, int B, int V, int Lmax) {
  extern __shared__ int gsm[];                 // start[V + 1] | pos[Lmax]
  int *start = gsm, *pos = gsm + V + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * GRAD_TCH, t1 = min(T, t0 + GRAD_TCH);
  const CtcLens len(in_len, tgt_len, b, T, Lmax);
  const bool bad = len.bad(), zero = !bad && zinf && nll[b] == INFINITY;
  const int Tb = bad ? 0 : zero ? 0 : len.Tb, L = bad ? 0 : len.L;
  const int64_t *tg = targets + (size_t)b * Lmax;
  if (!bad && t0 < Tb) {
    // class c (thread c) counts its label positions, a serial prefix sum over the V classes, then every class writes its positions
    for (int c = threadIdx.x; c < V; c += blockDim.x) {
      int n = 0;
      if (c != blank)
        for (int j = 0; j < L; ++j) n += (int)tg[j] == c;
      start[c + 1] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      start[0] = 0;
      for (int c = 0; c < V; ++c) start[c + 1] += start[c];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < V; c += blockDim.x) {
      int k = start[c];
      if (c != blank)
        for (int j = 0; j < L; ++j)
          if ((int)tg[j] == c) pos[k++] = j;
    }
    __syncthreads();
  }
  const int Smax = 2 * Lmax + 1;
  float gs = gscale[(size_t)b * gs_stride];
  if (mean) gs /= (float)B * (float)max(L, 1);
  for (int t = t0 + wave; t < t1; t += 4) {
    const size_t pair = (size_t)t * B + b;
    float *g = grad + pair * V;
    if (bad) {
      for (int c = lane; c < V; c += 64) g[c] = __uint_as_float(0x7fc00000u);
      continue;
    }
    if (t >= Tb) {                              // past the input, or an infeasible utterance under zero_infinity
      for (int c = lane; c < V; c += 64) g[c] = 0.0f;
      continue;
    }
    const float *abr = ab + pair * Smax;
    const float *btr = SEP ? bt + pair * Smax : nullptr;
    auto AB = [&](int s_) -> float { return SEP ? abr[s_] + btr[s_] : abr[s_]; };
    const float *lpr = lp + pair * V;
    const float n = nll[b];
    // blank: even states 0,2,..,2L
    Lse bl{-INFINITY, 0.0f};
    for (int j = lane; j <= L; j += 64) bl.add(AB(2 * j));
    const float M = wave_max(bl.m);
    float ssum = bl.m == -INFINITY ? 0.0f : bl.s * expf(bl.m - M);
    ssum = wave_sum(ssum);
    const float lcab0 = M == -INFINITY ? -INFINITY : M + logf(ssum);
    for (int c = lane; c < V; c += 64) {
      float lcab;
      if (c == blank) lcab = lcab0;
      else {
        Lse a{-INFINITY, 0.0f};
        for (int k = start[c]; k < start[c + 1]; ++k) a.add(AB(2 * pos[k] + 1));
        lcab = a.m == -INFINITY ? -INFINITY : a.m + logf(a.s);
      }
      const float l = lpr[c];
      g[c] = (expf(l) - expf(lcab + n - l)) * gs;
    }
  }
}

// Concatenated 1-D targets (torch's second layout) -> the padded (B, Lmax) rows the lattice reads, zero-filled past each length.  One
// workgroup per utterance; its offset is the exclusive prefix sum of the lengths before it (negative lengths count as 0: the lattice
// answers NaN for them), summed by the workgroup in a fixed order.  Nothing past flat[n_flat) is read.
__global__ __launch_bounds__(256) void ctc_pack_targets_kernel(const int64_t *__restrict__ flat, int64_t n_flat, const int64_t *__restrict__ tgt_len,
                                                               int64_t *__restrict__ padded, int Lmax) {
  __shared__ long long part[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long off = 0;
  for (int i = threadIdx.x; i < b; i += 256) off += tgt_len[i] > 0 ? tgt_len[i] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
  if (lane == 0) part[wave] = off;
  __syncthreads();
  off = part[0] + part[1] + part[2] + part[3];
  const int64_t L = tgt_len[b];
  int64_t *row = padded + (size_t)b * Lmax;
  for (int j = threadIdx.x; j < Lmax; j += 256) row[j] = (j < L && off + j < n_flat) ? flat[off + j] : 0;
}

// ---------------------------------------------------------------------------------------------------
// Forced alignment (ctcn_ctc_align): the alpha chain in the max-plus semiring plus a back-pointer trace.
//   v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if the loss allows the skip) + lp[t, ext(s)]   -- ONE float32 add, never fused
//   ties: the smallest move wins (a candidate replaces the best so far only if strictly greater), so the result is a function of the
//   input alone and a float32 restatement on the host is bit-identical.
// One workgroup per utterance; the forward chain is ctc_classic_walk with CtcMaxPolicy (state s = tid + k * CTC_THREADS, double-buffered LDS
// row, gathers PF frames ahead, one LDS barrier per frame).  The move of (t, s) is a 2-bit code; the 16 lanes tid & ~15 .. tid | 15 hold 16
// consecutive states, so two wave ballots hand the first lane of each group of 16 the packed word of its group (low bits in [0,16), high
// bits in [16,32)): one dword store per 16 states, no sub-dword write, no LDS atomic.  Rows of W = ceil(Smax / 16) words per frame live
//   BPLDS : in dynamic LDS behind the value rows (cfg2: 800 frames x 8 words = 25 KB), where the trace -- a chain of Tb dependent reads
//           walked by one lane -- pays LDS latency per frame;
//   else  : in the caller's workspace (B, T, W), brought back ALIGN_GWORDS words at a time by the whole workgroup for the lane to walk.
// The trace runs in chunks of up to ALIGN_CH frames: lane 0 writes the chunk's states into LDS, then the workgroup, a thread per frame, writes
// paths / frame_scores and the span ends (a state that differs from its neighbour in time).
// -DCTCN_ALIGN_FORWARD_ONLY (measurement builds, tools/align_bench.py): the kernel stops after the forward chain -- outputs are NOT valid.  The -1 / 0 fills of padding are stores issued
// before the chain, which never waits for them.
constexpr int ALIGN_CH = 1024;                     // frames per trace chunk (its states wait in LDS for the output phase)
constexpr int ALIGN_WALK = 8;                      // frames the walking lane takes per LDS round trip (2 * 7 < 16: two words per row cover them)
constexpr int ALIGN_GWORDS = 2048;                 // workspace branch: LDS words for the rows of a chunk (>= 8 frames at Smax = 4095)
constexpr size_t ALIGN_LDS_LIMIT = 64 * 1024;      // dynamic LDS of a launch that has not opted in to more (of the CU's 160 KB)

// The max-plus semiring of ctc_classic_walk: the best of the three moves (strictly greater replaces: the smallest move wins a tie) plus the
// log-prob, the move as the tag; a frame leaves its packed back-pointer words in `rows` (LDS or workspace, W words per frame).
struct CtcMaxPolicy {
  uint32_t *rows;
  int W, lane;
  __device__ __forceinline__ float prefetch(int, int) const { return 0.0f; }
  __device__ __forceinline__ void first(int, int, float) const {}
  __device__ __forceinline__ float combine(float x0, float x1, float x2, float q, int &code) const {
    float best = x0;
    if (x1 > best) { best = x1; code = 1; }
    if (x2 > best) { best = x2; code = 2; }
    return __fadd_rn(best, q);
  }
  // the two ballots run with every lane of the wave (code 0 in a lane past S)
  __device__ __forceinline__ void emit(int t, int s, bool live, float, int code, float) const {
    const int wsh = lane & 48;                      // this lane's group of 16 inside the two ballots
    const unsigned long long m0 = __ballot(code & 1), m1 = __ballot(code & 2);
    if ((lane & 15) == 0 && live)
      rows[(size_t)t * W + (s >> 4)] = (uint32_t)((m0 >> wsh) & 0xffffull) | ((uint32_t)((m1 >> wsh) & 0xffffull) << 16);
  }
};

template <int NS, bool BPLDS>
__global__ __launch_bounds__(CTC_THREADS) void ctc_align_kernel(const float *__restrict__ lp, const int64_t *__restrict__ targets,
                                                                const int64_t *__restrict__ in_len, const int64_t *__restrict__ tgt_len,
                                                                int32_t *__restrict__ paths, float *__restrict__ frame_scores,
                                                                float *__restrict__ score, int32_t *__restrict__ ok, int32_t *__restrict__ starts,
                                                                int32_t *__restrict__ ends, uint32_t *__restrict__ ws, int T, int B, int V, int Lmax,
                                                                int blank) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Smax = 2 * Lmax + 1, W = (Smax + 15) >> 4;
  const CtcLens len(in_len, tgt_len, b, T, Lmax);
  const bool bad = len.bad();
  const int Tb = bad ? 0 : len.Tb, L = bad ? 0 : len.L;
  int32_t *prow = paths + (size_t)b * T;
  float *frow = frame_scores + (size_t)b * T;
  int32_t *srow = starts ? starts + (size_t)b * Lmax : nullptr, *erow = ends ? ends + (size_t)b * Lmax : nullptr;
  // padding: frames past the input, tokens past the label
  for (int t = Tb + tid; t < T; t += CTC_THREADS) { prow[t] = -1; frow[t] = 0.0f; }
  for (int j = L + tid; j < Lmax; j += CTC_THREADS) {
    if (srow) srow[j] = -1;
    if (erow) erow[j] = -1;
  }
  auto no_alignment = [&](float sc) {
    for (int t = tid; t < Tb; t += CTC_THREADS) { prow[t] = -1; frow[t] = 0.0f; }
    for (int j = tid; j < L; j += CTC_THREADS) {
      if (srow) srow[j] = -1;
      if (erow) erow[j] = -1;
    }
    if (tid == 0) { score[b] = sc; ok[b] = 0; }
  };
  if (bad) { no_alignment(__uint_as_float(0x7fc00000u)); return; }
  if (Tb == 0) {
    if (L > 0) no_alignment(-INFINITY);
    else if (tid == 0) { score[b] = 0.0f; ok[b] = 1; }
    return;
  }
  const int S = len.S;
  int *ext = reinterpret_cast<int *>(smem + 2 * Smax);              // behind the walk's two value rows: ctc_classic_walk fills it
  int *st = ext + Smax;                                             // st[1 + i]: state at frame t0 + i of the chunk; st[0], st[n + 1]: its neighbours in time
  uint32_t *bpl = reinterpret_cast<uint32_t *>(st + ALIGN_CH + 2);  // BPLDS: row of frame t at bpl + t * W; else the rows of the current chunk
  uint32_t *bpg = BPLDS ? nullptr : ws + (size_t)b * T * W;         // row of frame t at bpg + t * W
  const CtcMaxPolicy pol{BPLDS ? bpl : bpg, W, tid & 63};
  const float *prev = ctc_classic_walk<1, NS>(smem, lp, targets, Tb, S, B, V, Lmax, blank, pol);
  __syncthreads();           // the last value row, every back-pointer row (LDS or workspace) and the fills are done
  const float l1 = prev[S - 1], l2 = S > 1 ? prev[S - 2] : -INFINITY;
  const bool second = S > 1 && l2 > l1;
  const float sc = second ? l2 : l1;
  if (sc == -INFINITY) { no_alignment(sc); return; }
  if (tid == 0) { score[b] = sc; ok[b] = 1; }
#ifdef CTCN_ALIGN_FORWARD_ONLY
  return;
#endif
  const int CH = BPLDS ? ALIGN_CH : min(ALIGN_CH, ALIGN_GWORDS / W);
  int s = second ? S - 2 : S - 1, s_above = -1;     // the walk's state: meaningful in thread 0 only
  for (int t1 = Tb; t1 > 0;) {
    const int n = min(t1, CH), t0 = t1 - n;
    if (!BPLDS)
      for (int i = tid; i < n * W; i += CTC_THREADS) bpl[i] = bpg[(size_t)t0 * W + i];
    __syncthreads();
    if (tid == 0) {
      const uint32_t *rows = BPLDS ? bpl + (size_t)t0 * W : bpl;
      st[n + 1] = s_above;
      // ALIGN_WALK frames per LDS round trip: the state drops by at most 2 per frame, so over 8 frames it stays inside the word of s and
      // the word below it -- both are fetched for the 8 rows at once and the 8 dependent steps run in registers
      for (int i = n - 1; i >= 0; i -= ALIGN_WALK) {
        const int wi = s >> 4, wl = max(wi - 1, 0);
        uint32_t hi[ALIGN_WALK], lo[ALIGN_WALK];
#pragma unroll
        for (int k = 0; k < ALIGN_WALK; ++k) {
          const uint32_t *row = rows + (size_t)max(i - k, 0) * W;
          hi[k] = row[wi];
          lo[k] = row[wl];
        }
#pragma unroll
        for (int k = 0; k < ALIGN_WALK; ++k) {
          if (i - k >= 0) {
            st[i - k + 1] = s;
            if (i - k == 0) s_above = s;
            if (t0 + i - k > 0) {                   // frame 0 has no predecessor (and no row)
              const uint32_t w = ((s >> 4) == wi ? hi[k] : lo[k]) >> (s & 15);
              s -= (int)((w & 1u) | ((w >> 15) & 2u));
            }
          }
        }
      }
      st[0] = t0 > 0 ? s : -1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += CTC_THREADS) {
      const int t = t0 + i, si = st[i + 1];
      const int c = ext[si];
      prow[t] = c;
      frow[t] = lp[((size_t)t * B + b) * V + c];
      if (si & 1) {
        if (srow && st[i] != si) srow[si >> 1] = t;
        if (erow && st[i + 2] != si) erow[si >> 1] = t + 1;
      }
    }
    t1 = t0;
  }
}

}  // namespace

// ---- Plans: what a call launches, by arithmetic on its shapes and the options alone; the launches below only carry a plan out ----

// The lattice passes of every CTC entry point: alpha alone (ctcn_ctc_fwd, ctcn_ctc_fwd_ex without beta), the beta pass added into alpha
// in place (ctcn_ctc_bwd's one-buffer reserve), or alpha and beta side by side in one launch (ctcn_ctc_fwd_both, ctcn_ctc_fwd_ex).
enum CtcPasses { CTC_ALPHA, CTC_BETA_INTO_ALPHA, CTC_ALPHA_BETA };

// The launch of a lattice pass (ctcn_diag_ctc_lattice_plan shows it to the CPU tests).  Skewed (ctc_lattices_skew_kernel: a
// state per lane on `waves` waves of 64, the ring and the two final states in LDS) where the lattice fits CTC_SKEW_WAVES waves and option
// "ctc_lattice_skew" is on; otherwise the classic kernels: CTC_THREADS threads, ns states per thread, three lattice rows of LDS.
struct CtcLatticeOptions { int skew; };
struct CtcLatticePlan { int skewed, waves, ns, threads; size_t lds; };
CtcLatticePlan plan_ctc_lattice(int Lmax, const CtcLatticeOptions &o) {
  const int S = 2 * Lmax + 1;
  CtcLatticePlan p;
  p.waves = ceil_div(S, 64);
  p.skewed = o.skew && p.waves <= CTC_SKEW_WAVES;
  if (p.skewed) {
    p.ns = 1;
    p.threads = 64 * p.waves;
    p.lds = (size_t)(8 * CTC_RING * p.waves + 2) * sizeof(float);
  } else {
    const int ns = ceil_div(S, CTC_THREADS);
    p.ns = ns <= 1 ? 1 : ns <= 2 ? 2 : ns <= 4 ? 4 : ns <= 8 ? 8 : 16;
    p.threads = CTC_THREADS;
    p.lds = (size_t)(3 * S) * sizeof(float);
  }
  return p;
}

// The launch of ctcn_ctc_align: the classic walk's ns, and where the back-pointer rows (ceil(Smax / 16) words per frame) live -- in LDS behind
// the walk's three rows and the trace chunk's states where all T of them fit ALIGN_LDS_LIMIT, else in the caller's workspace of ws_bytes with
// ALIGN_GWORDS words of LDS to bring them back through.  The same (T, Lmax) always takes the same branch.
struct CtcAlignPlan { bool rows_in_lds; int ns; size_t lds, ws_bytes; };
static CtcAlignPlan plan_ctc_align(int T, int B, int Lmax) {
  const int S = 2 * Lmax + 1;
  const size_t fixed = (size_t)(3 * S + ALIGN_CH + 2) * sizeof(float), rows = (size_t)T * ceil_div(S, 16) * sizeof(uint32_t);
  CtcAlignPlan p;
  p.rows_in_lds = fixed + rows <= ALIGN_LDS_LIMIT;
  p.ns = plan_ctc_lattice(Lmax, CtcLatticeOptions{0}).ns;
  p.lds = fixed + (p.rows_in_lds ? rows : (size_t)ALIGN_GWORDS * sizeof(uint32_t));
  p.ws_bytes = p.rows_in_lds ? 0 : (size_t)B * rows;
  return p;
}

// f(std::integral_constant<int, NS>{}) for a plan's ns: the instantiations of the classic walk (1, 2, 4, 8 or CTC_NS states per thread)
template <class F>
static void with_ctc_ns(int ns, F &&f) {
  switch (ns) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, CTC_NS>{}); break;
  }
}

static bool ctc_label_too_long(const char *who, int Lmax) {
  if (2 * Lmax + 1 <= CTC_THREADS * CTC_NS) return false;
  ctcn_set_error("%s: label length %d > %d unsupported", who, Lmax, (CTC_THREADS * CTC_NS - 1) / 2);
  return true;
}

static int ctc_lattices(const char *who, CtcPasses passes, const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len,
                        float *alpha, float *beta, float *nll, int T, int B, int V, int Lmax, int blank, hipStream_t st) {
  if (ctc_label_too_long(who, Lmax)) return CTCN_EUNSUPPORTED;
  CtcLatticeOptions opt{ctcn_get_option("ctc_lattice_skew")};
  if (passes == CTC_BETA_INTO_ALPHA) opt.skew = 0;          // the in-place beta pass has no skewed body
  const CtcLatticePlan plan = plan_ctc_lattice(Lmax, opt);
  const dim3 grid(B, passes == CTC_ALPHA_BETA ? 2 : 1), block(plan.threads);
  if (plan.skewed) {                                        // CTC_ALPHA or CTC_ALPHA_BETA, by the grid
    const int slow = ctcn_get_option("ctc_slow_wave");
    hipLaunchKernelGGL(slow ? ctc_lattices_skew_kernel<true> : ctc_lattices_skew_kernel<false>, grid, block, plan.lds, st, lp, targets, in_len,
                       tgt_len, alpha, beta, nll, T, B, V, Lmax, blank, slow);
  } else {
    with_ctc_ns(plan.ns, [&](auto ns) {
      constexpr int NS = decltype(ns)::value;
      switch (passes) {
        case CTC_ALPHA:
          hipLaunchKernelGGL((ctc_lattice_kernel<1, NS>), grid, block, plan.lds, st, lp, targets, in_len, tgt_len, alpha, nll, T, B, V, Lmax, blank);
          break;
        case CTC_BETA_INTO_ALPHA:
          hipLaunchKernelGGL((ctc_lattice_kernel<-1, NS>), grid, block, plan.lds, st, lp, targets, in_len, tgt_len, alpha, (float *)nullptr, T, B, V,
                             Lmax, blank);
          break;
        case CTC_ALPHA_BETA:
          hipLaunchKernelGGL((ctc_lattices_kernel<NS>), grid, block, plan.lds, st, lp, targets, in_len, tgt_len, alpha, beta, nll, T, B, V, Lmax,
                             blank);
          break;
      }
    });
  }
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

// The gradient of every CTC entry point.  beta == NULL: alpha holds alpha + beta (ctcn_ctc_bwd's in-place reserve).
static int ctc_grad(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, const float *alpha,
                    const float *beta, const float *nll, const float *gscale, int gs_stride, int reduction, int zero_infinity, int blank,
                    float *grad_lp, int T, int B, int V, int Lmax, hipStream_t st) {
  const size_t sm = (size_t)(V + 1 + Lmax) * sizeof(int);
  const int mean = reduction == CTCN_REDUCTION_MEAN, zinf = zero_infinity != 0;
  hipLaunchKernelGGL(beta ? ctc_grad_kernel<true> : ctc_grad_kernel<false>, dim3(ceil_div(T, GRAD_TCH), B), dim3(256), sm, st, lp, targets, in_len,
                     tgt_len, alpha, beta, nll, gscale, gs_stride, mean, zinf, blank, grad_lp, T, B, V, Lmax);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

// ---- The entry points (contracts in include/ctcn.h) ----

extern "C" int ctcn_log_softmax_fwd(const float *logits, float *lp, int32_t *argmax, int rows, int V, void *stream) {
  CTCN_REQUIRE(logits && lp && rows > 0 && V > 0, "ctcn_log_softmax_fwd: bad args");
  hipLaunchKernelGGL((log_softmax_kernel<true>), dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, logits, lp, argmax, rows, V);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
extern "C" int ctcn_argmax(const float *lp, int32_t *argmax, int rows, int V, void *stream) {
  CTCN_REQUIRE(lp && argmax && rows > 0 && V > 0, "ctcn_argmax: bad args");
  hipLaunchKernelGGL((log_softmax_kernel<false>), dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, lp, (float *)nullptr, argmax, rows, V);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
extern "C" int ctcn_log_softmax_bwd(const float *lp, const float *dlp, float *dlogits, int rows, int V, void *stream) {
  CTCN_REQUIRE(lp && dlp && dlogits && rows > 0 && V > 0, "ctcn_log_softmax_bwd: bad args");
  hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, lp, dlp, dlogits, rows, V);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_ctc_pack_targets(const int64_t *flat, int64_t n_flat, const int64_t *tgt_len, int64_t *padded, int B, int Lmax, void *stream) {
  CTCN_REQUIRE(tgt_len && padded && (flat || n_flat == 0) && n_flat >= 0 && B > 0 && Lmax > 0, "ctcn_ctc_pack_targets: bad args");
  hipLaunchKernelGGL(ctc_pack_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, flat, n_flat, tgt_len, padded, Lmax);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_diag_ctc_lattice_plan(int Lmax, int *out) {
  CTCN_REQUIRE(out && Lmax >= 0 && 2 * (int64_t)Lmax + 1 <= CTC_THREADS * CTC_NS, "ctcn_diag_ctc_lattice_plan: bad args");
  const CtcLatticePlan p = plan_ctc_lattice(Lmax, CtcLatticeOptions{ctcn_get_option("ctc_lattice_skew")});
  out[0] = p.skewed; out[1] = p.waves; out[2] = p.ns; out[3] = p.threads; out[4] = (int)p.lds; out[5] = CTC_SKEW * CTC_CHUNK;
  return CTCN_OK;
}

extern "C" int ctcn_ctc_fwd(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, float *alpha,
                            float *nll, int T, int B, int V, int Lmax, void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && alpha && nll && (targets || Lmax == 0), "ctcn_ctc_fwd: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0, "ctcn_ctc_fwd: bad dims");
  return ctc_lattices("ctcn_ctc_fwd", CTC_ALPHA, lp, targets, in_len, tgt_len, alpha, nullptr, nll, T, B, V, Lmax, 0, (hipStream_t)stream);
}

extern "C" int ctcn_ctc_bwd(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, float *alpha,
                            const float *nll, const float *gscale, float *grad_lp, int T, int B, int V, int Lmax, void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && alpha && nll && gscale && grad_lp && (targets || Lmax == 0), "ctcn_ctc_bwd: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0, "ctcn_ctc_bwd: bad dims");
  hipStream_t st = (hipStream_t)stream;
  const int rc = ctc_lattices("ctcn_ctc_bwd", CTC_BETA_INTO_ALPHA, lp, targets, in_len, tgt_len, alpha, nullptr, nullptr, T, B, V, Lmax, 0, st);
  if (rc != CTCN_OK) return rc;
  return ctc_grad(lp, targets, in_len, tgt_len, alpha, nullptr, nll, gscale, 0, CTCN_REDUCTION_SUM, 0, 0, grad_lp, T, B, V, Lmax, st);
}

extern "C" int ctcn_ctc_fwd_both(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, float *alpha,
                                 float *beta, float *nll, int T, int B, int V, int Lmax, void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && alpha && beta && nll && (targets || Lmax == 0), "ctcn_ctc_fwd_both: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0, "ctcn_ctc_fwd_both: bad dims");
  return ctc_lattices("ctcn_ctc_fwd_both", CTC_ALPHA_BETA, lp, targets, in_len, tgt_len, alpha, beta, nll, T, B, V, Lmax, 0, (hipStream_t)stream);
}

extern "C" int ctcn_ctc_grad(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, const float *alpha,
                             const float *beta, const float *nll, const float *gscale, float *grad_lp, int T, int B, int V, int Lmax,
                             void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && alpha && beta && nll && gscale && grad_lp && (targets || Lmax == 0), "ctcn_ctc_grad: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0, "ctcn_ctc_grad: bad dims");
  return ctc_grad(lp, targets, in_len, tgt_len, alpha, beta, nll, gscale, 0, CTCN_REDUCTION_SUM, 0, 0, grad_lp, T, B, V, Lmax, (hipStream_t)stream);
}

extern "C" int ctcn_ctc_fwd_ex(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, float *alpha,
                               float *beta, float *nll, int T, int B, int V, int Lmax, int blank, void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && alpha && nll && (targets || Lmax == 0), "ctcn_ctc_fwd_ex: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0 && alpha != beta, "ctcn_ctc_fwd_ex: bad dims");
  CTCN_REQUIRE(blank >= 0 && blank < V, "ctcn_ctc_fwd_ex: blank %d outside [0, %d)", blank, V);
  return ctc_lattices("ctcn_ctc_fwd_ex", beta ? CTC_ALPHA_BETA : CTC_ALPHA, lp, targets, in_len, tgt_len, alpha, beta, nll, T, B, V, Lmax, blank,
                      (hipStream_t)stream);
}

extern "C" int ctcn_ctc_grad_ex(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, const float *alpha,
                                const float *beta, const float *nll, const float *gscale, int gscale_stride, int reduction, int zero_infinity,
                                int blank, float *grad_lp, int T, int B, int V, int Lmax, void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && alpha && nll && gscale && grad_lp && (targets || Lmax == 0), "ctcn_ctc_grad_ex: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0, "ctcn_ctc_grad_ex: bad dims");
  CTCN_REQUIRE(blank >= 0 && blank < V, "ctcn_ctc_grad_ex: blank %d outside [0, %d)", blank, V);
  CTCN_REQUIRE(reduction == CTCN_REDUCTION_NONE || reduction == CTCN_REDUCTION_MEAN || reduction == CTCN_REDUCTION_SUM,
               "ctcn_ctc_grad_ex: reduction %d", reduction);
  CTCN_REQUIRE(gscale_stride == 0 || gscale_stride == 1, "ctcn_ctc_grad_ex: gscale_stride %d (0 or 1)", gscale_stride);
  return ctc_grad(lp, targets, in_len, tgt_len, alpha, beta, nll, gscale, gscale_stride, reduction, zero_infinity, blank, grad_lp, T, B, V,
                  Lmax, (hipStream_t)stream);
}

extern "C" size_t ctcn_ctc_align_ws_bytes(int T, int B, int Lmax) {
  if (T <= 0 || B <= 0 || Lmax < 0) return 0;
  return plan_ctc_align(T, B, Lmax).ws_bytes;
}

extern "C" int ctcn_ctc_align(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, int32_t *paths,
                              float *frame_scores, float *score, int32_t *ok, int32_t *starts, int32_t *ends, int T, int B, int V, int Lmax,
                              int blank, void *ws, size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(lp && in_len && tgt_len && paths && frame_scores && score && ok && (targets || Lmax == 0), "ctcn_ctc_align: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 0 && Lmax >= 0, "ctcn_ctc_align: bad dims");
  CTCN_REQUIRE(blank >= 0 && blank < V, "ctcn_ctc_align: blank %d outside [0, %d)", blank, V);
  if (ctc_label_too_long("ctcn_ctc_align", Lmax)) return CTCN_EUNSUPPORTED;
  const CtcAlignPlan plan = plan_ctc_align(T, B, Lmax);
  if (!plan.rows_in_lds) {
    CTCN_REQUIRE(ws && ((uintptr_t)ws & 3) == 0, "ctcn_ctc_align: workspace of ctcn_ctc_align_ws_bytes needed (T %d, Lmax %d), 4-byte aligned", T, Lmax);
    if (ws_bytes < plan.ws_bytes) { ctcn_set_error("ctcn_ctc_align: workspace %zu < %zu bytes", ws_bytes, plan.ws_bytes); return CTCN_EWORKSPACE; }
  }
  with_ctc_ns(plan.ns, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    hipLaunchKernelGGL((plan.rows_in_lds ? ctc_align_kernel<NS, true> : ctc_align_kernel<NS, false>), dim3(B), dim3(CTC_THREADS), plan.lds,
                       (hipStream_t)stream, lp, targets, in_len, tgt_len, paths, frame_scores, score, ok, starts, ends, (uint32_t *)ws, T, B, V, Lmax,
                       blank);
  });
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

