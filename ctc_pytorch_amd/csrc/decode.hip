// decode.hip -- CTC prefix beam search with a bigram or trigram LM, one workgroup per utterance (gfx950).
//
// replaces: BeamDecoder.decode -> ctcBeamSearch.decode (reference timit/utils/ctcDecoder.py:181-192,
// timit/utils/BeamSearch.py:73-153 with log_add_prob :43-50, calcExtPr :52-66, BeamState.sort :29-33,
// BeamState.norm :23-27) and LanguageModel.get_bi_prob (timit/utils/NgramLM.py:65-78, pre-tabulated on the
// host into lm[(V+1)*(V+1)]).  Semantics reproduced exactly:
//   * scores are IEEE double in the ln domain with the LOG_ZERO = -99999999.0 sentinel rules of log_add_prob;
//   * the frame-skip test (1 - p_blank < 0.1) and the repeat rule (p_blank[t-1] < 0.9) are float32 compares;
//   * the python dict of labellings is modelled by a prefix trie (labelling == node id, children found
//     through an open-addressing table in the workspace), so equal labellings reached along different
//     paths merge exactly as dict keys do; the merged entry takes the insertion position of its first touch
//     and accumulates its contributions in the reference's visiting order;
//   * BHat = first W entries of a stable descending sort == W rounds of arg-max with (score desc,
//     insertion index asc) ordering over the <= W*V candidate entries of the step;
//   * the reference's two failure modes are reported, not hidden: status 1 = an empty labelling reaches the
//     final LM step (python IndexError at BeamSearch.py:135), status 2 = log of a zero probability
//     (python ValueError).
// LM order (ctcn_beam_decode_lm): the order is a property of the call and a template parameter of the kernels.  Order 2 is the reference's
// term lm[c1][k]; order 3 -- which the reference's LanguageModel(n_gram=3) accepts and never evaluates -- replaces it, in calcExtPr and in
// the final step, by tri[c0][c1][k] over a dense (V+1)^3 table (index V = '<s>' for c0 / c1, '</s>' for k): tri[V][V][k] for the empty
// labelling, tri[V][y[0]][k] for one class, tri[y[-2]][y[-1]][k] beyond.  Every beam slot therefore carries the class before its last
// (generic kernel: BeamState::prev; fast kernel: z_plast, mirrored to bm_c0 for the candidate waves), and the fast kernel's wave 0 one
// more (z_pplast) because it recomputes the PARENT's extension term.  The order-3 table is read from global memory on every path and the
// product with alpha is rounded on its own (lm_scaled), so all paths agree to the bit; the order-2 instantiations compile to the code they
// were (same VGPRs, SGPRs, LDS and scratch: DESIGN.md section 7s).
// Parallelism: utterances across workgroups (replicas, no collective), candidates (beam x class) across the
// 256 lanes of the workgroup; every per-step quantity lives in LDS (beam state, log-probs, candidate scores).
#include <algorithm>

#include "common.h"

namespace {

// Widest beam of the generic kernel: its beam state lives in dynamic LDS sized for the call's width (GenericLds: 146 KB at W = 1 024, which
// gfx950's 160 KB per workgroup still hold); beyond that the state would have to live in global memory.
constexpr int BEAM_WMAX = 1024;
constexpr double LOG_ZERO = -99999999.0;
constexpr unsigned long long HT_EMPTY = ~0ull;

__device__ __forceinline__ double log_add_prob(double log_x, double log_y) {   // BeamSearch.py:43-50
  if (log_x <= LOG_ZERO) return log_y;
  if (log_y <= LOG_ZERO) return log_x;
  if ((log_y - log_x) > 0.0) { const double t = log_x; log_x = log_y; log_y = t; }
  return log_x + log(1 + exp(log_y - log_x));
}

// ln P_LM * alpha rounded on its own before it joins a sum -- as the fast kernel's LDS table holds it and as the reference computes it.  Without
// the pragma the compiler fuses the product into the sum (v_fma_f64) wherever it is formed per use: the fast kernel's global-memory LM variant
// then differed from its LDS variant in the last bits (beam_occ2 = 1 / 2 where the LM does not fit beside the trie, V > 70 at any setting), and
// the generic kernel from both (tests/test_beam_edges.py holds every path to the same bits).
__device__ __forceinline__ double lm_scaled(double lm, double alpha) {
#pragma clang fp contract(off)
  return lm * alpha;
}

struct Fields { double nb, b, t; };
__device__ __forceinline__ void apply_stay(Fields &e, double s_nb, double s_b) {   // BeamSearch.py:108-113
  e.nb = log_add_prob(e.nb, s_nb);
  e.b = log_add_prob(e.b, s_b);
  const double tot = log_add_prob(s_b, s_nb);
  e.t = log_add_prob(e.t, tot);
}
__device__ __forceinline__ void apply_ext(Fields &e, double pr) {                  // BeamSearch.py:122-125
  e.nb = log_add_prob(e.nb, pr);
  e.t = log_add_prob(e.t, pr);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
  return x;
}

struct BeamState {   // one copy of the beam (BHat) in LDS: arrays of `wcap` entries carved out of the kernel's dynamic shared memory
  int *node, *len, *last, *par;
  double *pB, *pNB, *pT;
  int *prev;   // order 3 only: the class before `last` (y[-2]; meaningful where len >= 2)
};

struct BeamArgs {
  const float *x; int input_is_prob; const int32_t *lens; const double *lm; double alpha; int W, blank;
  int32_t *out_ids, *out_len; double *out_score; int32_t *status; int T, B, V;
  int nbest; int32_t *out_count;        // ctcn_beam_decode_nbest: the `nbest` best labellings per utterance (outputs [B][nbest]...), their number in out_count
  unsigned long long *ht_keys; int *ht_ids; int *node_par; int *node_sym; double *cand_global;
  int *node_slot, *cand_owner;   // beam_kernel: beam slot of a trie node / beam slot whose labelling merges with a candidate (lookups that replace scans of the beam)
  int ht_size, max_nodes, cand_in_lds;
  int wcap, smax;       // beam_kernel: capacity of the beam-state arrays (W rounded up to 64) and of the selection's survivor list
  int bitonic;          // beam_kernel: rank up to 256 survivors by a bitonic sort (option beam_bitonic, default 1) instead of counting pairs
  int lm_in_lds;        // beam_kernel: the (V+1)^2 ln-prob table is copied into dynamic LDS behind the state arrays (when the launch's budget holds it)
#ifdef CTCN_BEAM_STATS
  long long *stats;     // development instrumentation (tools/mb_beam.py generic): cycles per phase of workgroup 0, thread 0
#endif
};
#ifdef CTCN_BEAM_STATS
#define GSTAMP(i) do { if (c.b == 0 && c.tid == 0) { const long long now_ = clock64(); c.gst[i] += now_ - c.glast; c.glast = now_; } } while (0)
#else
#define GSTAMP(i) do { } while (0)
#endif

// ---- What both kernels share: candidate order and columns, key maps, arg-max rounds, the final step, the two dynamic-LDS layouts ----
__device__ __forceinline__ bool cand_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }
// a beam slot's row of the candidate table: column 0 = the stay entry, column kk >= 1 = the kk-th non-blank class; cand_class(0, blank) = -1
__device__ __forceinline__ int cand_class(int kk, int blank) { return (kk - 1 < blank) ? kk - 1 : kk; }
__device__ __forceinline__ int class_col(int k, int blank) { return (k < blank) ? k + 1 : k; }
// Order-preserving maps double -> uint64 (v > w <=> key(v) > key(w); no NaN among the scores; never 0 for a finite value), in two forms:
//   f64_key / key_f64  a bijection.  The fast kernel carries its candidates as keys and reads the SCORES back with key_f64: folding a zero
//                      there would change result bits.  The generic kernel turns its pruning bound back into a double with it.
//   dkey               folds -0.0 onto +0.0, which compare equal as doubles.  The generic kernel compares keys with keys (bound search,
//                      bitonic ranks) and reads every score from the candidate table, never from a key.
__device__ __forceinline__ unsigned long long f64_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_f64(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ unsigned long long dkey(double v) { return f64_key(v == 0.0 ? 0.0 : v); }
// W block-wide arg-max rounds over the candidate table under cand_better(): the selection's fallback in both kernels (more survivors than
// their list holds: exact ties by the hundred).  All NT threads; `barrier` and `wave` are the kernel's own; red_i has NT / 64 + 1 entries.
// Round r's winner goes to sel[r] / selv[r] and on_pick(r).  `v != -inf` selects what `v > -inf` does: a NaN never passes cand_better().
template <int NT, typename Barrier, typename OnPick>
__device__ __forceinline__ int arg_max_rounds(double *cand, int ncand, int W, double *red_v, int *red_i, int *sel, double *selv, int wave,
                                              Barrier barrier, OnPick on_pick) {
  constexpr int NWV = NT / 64, NONE = 0x7fffffff;
  const int tid = threadIdx.x, lane = tid & 63;
  int got = 0;
  for (int r = 0; r < W; ++r) {
    double bv = -INFINITY; int bi = NONE;
    for (int c = tid; c < ncand; c += NT) {
      const double v = cand[c];
      if (v != -INFINITY && cand_better(v, c, bv, bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != NONE && (bi == NONE || cand_better(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    barrier();
    if (tid == 0) {
      double v = red_v[0]; int ix = red_i[0];
      for (int w = 1; w < NWV; ++w)
        if (red_i[w] != NONE && (ix == NONE || cand_better(red_v[w], red_i[w], v, ix))) { v = red_v[w]; ix = red_i[w]; }
      red_i[NWV] = ix;
      if (ix != NONE) { sel[r] = ix; selv[r] = v; on_pick(r); cand[ix] = -INFINITY; }
    }
    barrier();
    if (red_i[NWV] == NONE) break;
    ++got;
  }
  return got;
}
// The final step (BeamSearch.py:130-151), thread 0: the end-of-sentence LM term, length normalisation (:147), then `last.sort()[0:nbest]`
// (:150, the reference keeps [0]) -- a stable descending sort: among equal scores the earlier entry of BHat comes first -- and every picked
// labelling read back through the trie: walk(n) returns the last class of node n and moves n to its parent.  pT is reused for the scores and
// `taken` for the picks (it may be `last`: entry r's last class is read before taken[r] is written).  Status 1 / 3 or != 0: outputs zeroed.
// ORDER 3: the end term is tri[c0][last][V], c0 = prev[r] (the class before the last) for a labelling of two classes or more, V (<s>) for one.
template <int ORDER = 2, typename Args, typename Walk>
__device__ __forceinline__ void beam_finish(const Args &a, int b, int status, bool too_many_nodes, int nb, const int *len, const int *last,
                                            const int *node, double *pT, int *taken, const double *lm, Walk walk, const int *prev = nullptr) {
  if (threadIdx.x != 0) return;
  const int NB = a.nbest, V = a.V, T = a.T;
  int nout = 0;
  if (status == 0) {
    for (int r = 0; r < nb; ++r) if (len[r] == 0) status = 1;         // classes[y[-1]] on () -> IndexError
    if (too_many_nodes) status = 3;
  }
  if (status == 0) {
    for (int r = 0; r < nb; ++r) {
      // (the reference's log_add_prob(LOG_ZERO, pr): its first test returns the second argument, BeamSearch.py:44-45)
      const int ln = len[r];
      size_t row = (size_t)last[r];
      if (ORDER == 3) row += (size_t)(ln > 1 ? prev[r] : V) * (V + 1);
      const double tot = pT[r] + lm_scaled(lm[row * (V + 1) + V], a.alpha);
      pT[r] = tot * (1.0 / (ln ? ln : 1));
      taken[r] = 0;
    }
    nout = min(NB, nb);
    for (int k = 0; k < nout; ++k) {
      int best = -1; double bestv = 0.0;
      for (int r = 0; r < nb; ++r)
        if (!taken[r] && (best < 0 || pT[r] > bestv)) { best = r; bestv = pT[r]; }
      taken[best] = 1;
      const int ln = len[best];
      const size_t o = (size_t)b * NB + k;
      a.out_len[o] = ln; a.out_score[o] = bestv;
      int n = node[best];
      for (int i = ln - 1; i >= 0; --i) a.out_ids[o * T + i] = walk(n);
    }
  }
  for (int k = nout; k < NB; ++k) { a.out_len[(size_t)b * NB + k] = 0; a.out_score[(size_t)b * NB + k] = 0.0; }
  if (a.out_count) a.out_count[b] = nout;
  a.status[b] = status;
}
// Dynamic LDS of beam_kernel, byte offsets: lg[V] doubles | cand[W * V] doubles (cand_in_lds) | STATE x wcap + smax doubles | as many ints |
// LM table (lm_in_lds).  Doubles: 2 x {pB, pNB, pT}, sNB, sB, sT, selv (wcap each), sv_v (smax); ints: 2 x {node, len, last, par}, mfrom, sel,
// sv_i -- BeamCtx::carve names them.  Order 3 adds 2 x prev (wcap ints each) behind sv_i and keeps its (V+1)^3 table in global memory.
struct GenericLds {
  static constexpr int STATE = 10;
  size_t cand, dbl, ints, lm, total;
  __host__ __device__ GenericLds(int V, int W, int wcap, int smax, bool cand_in_lds, bool lm_in_lds, int order = 2) {
    size_t off = (size_t)V * sizeof(double);
    cand = off; off += cand_in_lds ? (size_t)W * V * sizeof(double) : 0;
    dbl = off;  off += ((size_t)STATE * wcap + smax) * sizeof(double);
    ints = off; off += ((size_t)STATE * wcap + smax) * sizeof(int);
    if (order == 3) off += (size_t)2 * wcap * sizeof(int);
    lm = (off + 7) & ~(size_t)7;                                     // (8 bytes of room for that rounding)
    total = off + (lm_in_lds ? table_bytes(V) : 0);
  }
  static __host__ __device__ size_t table_bytes(int V) { return (size_t)(V + 1) * (V + 1) * sizeof(double) + 8; }
};
// Dynamic LDS of the fast kernel: alpha * LM (V+1)^2 doubles (lm_lds) | cand[W * V] doubles | lg[2][V] doubles (by frame parity) |
// mslot[W * V] ints | flist[T] ints | trie[trie_slots] uints.  Off: size_t in the plan, which sizes any shape; unsigned in the kernel, which
// sits at its register limit and takes W <= 60, V <= 256, T < 2^22 only.
template <typename Off>
struct FastLdsT {
  Off cand, lg2, mslot, flist, trie, total;
  __host__ __device__ FastLdsT(int T, int V, int W, bool lm_lds, int trie_slots) {
    Off off = lm_lds ? (Off)table_bytes(V) : 0;
    cand = off;  off += (Off)W * V * (Off)sizeof(double);
    lg2 = off;   off += (Off)2 * V * (Off)sizeof(double);
    mslot = off; off += (Off)W * V * (Off)sizeof(int);
    flist = off; off += (Off)T * (Off)sizeof(int);
    trie = off;  off += (Off)trie_slots * (Off)sizeof(unsigned);
    total = off;
  }
  static __host__ __device__ size_t table_bytes(int V) { return (size_t)(V + 1) * (V + 1) * sizeof(double); }
};

// Sum / 64-bit maximum over each row of 16 lanes by DPP (no LDS crossbar: a ds_bpermute butterfly is a chain of ~150-cycle hops under load);
// afterwards every lane of a row holds the row's result
__device__ __forceinline__ int row16_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);     // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);     // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);    // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);    // row_mirror
  return v;
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max_u64_step(unsigned long long x) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(x & 0xffffffffull), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), CTRL, 0xf, 0xf, true);
  const unsigned long long o = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
  return o > x ? o : x;
}
__device__ __forceinline__ unsigned long long row16_max_u64(unsigned long long x) {
  x = dpp_max_u64_step<0xB1>(x);
  x = dpp_max_u64_step<0x4E>(x);
  x = dpp_max_u64_step<0x141>(x);
  x = dpp_max_u64_step<0x140>(x);
  return x;
}
// 32-bit maximum over each row of 16 lanes (row_shr 1 / 2 / 4 / 8: lanes without a source keep their own value); only LANE 15 of a row holds
// the row's result
template <int CTRL>
__device__ __forceinline__ unsigned dpp_umax_step(unsigned v) {
  const unsigned s = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
  return max(v, s);
}
__device__ __forceinline__ unsigned row16_umax(unsigned v) {
  v = dpp_umax_step<0x111>(v);
  v = dpp_umax_step<0x112>(v);
  v = dpp_umax_step<0x114>(v);
  v = dpp_umax_step<0x118>(v);
  return v;
}
__device__ __forceinline__ int wave_sum_rows(int v) {               // wave-wide sum, uniform result
  v = row16_sum(v);
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// Lane i <- lane i ^ J of a 32-bit value without the LDS crossbar: DPP quad permutes / row rotation inside a row of 16 lanes, the gfx950
// v_permlane16_swap / v_permlane32_swap across rows and halves (swap(x, x): result 0 holds the lower partner's rows, result 1 the upper's).
// J = 4 has no single pattern: both row shifts by 4 are taken and `pick_shl` (probed once by the caller: which of the two reads lane i ^ 4)
// selects.
template <int J>
__device__ __forceinline__ unsigned xor_lane(unsigned x, int lane, bool pick_shl) {
  if (J == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true);       // quad_perm [1,0,3,2]
  if (J == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, true);       // quad_perm [2,3,0,1]
  if (J == 4) {
    const unsigned a = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xf, 0xf, true);    // row_shl:4
    const unsigned c = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);    // row_shr:4
    return pick_shl ? a : c;
  }
  if (J == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, true);      // row_ror:8
  if (J == 16) { const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false); return (lane & 16) ? r[0] : r[1]; }
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return (lane & 32) ? r[0] : r[1];
}
// (key a, index ia) sorts before (key b, index ib): key descending, index ascending.  (A 96-bit subtract-with-borrow chain through
// __builtin_subc was measured: slower than what hipcc makes of the two 64-bit compares.)
__device__ __forceinline__ bool elem_before(unsigned ahi, unsigned alo, int ia, unsigned bhi, unsigned blo, int ib) {
  const unsigned long long ka = ((unsigned long long)ahi << 32) | alo, kb = ((unsigned long long)bhi << 32) | blo;
  return ka > kb || (ka == kb && ia < ib);
}
// one compare-exchange step of the bitonic network on (64-bit key descending, index ascending) elements, partner lane ^ J; `keep_better`:
// this lane keeps the better element of the pair.  Equal elements (only the padding) may swap: they are identical.
template <int J>
__device__ __forceinline__ void bitonic_step(unsigned &khi, unsigned &klo, int &ix, bool keep_better, int lane, bool pick_shl) {
  const unsigned ohi = xor_lane<J>(khi, lane, pick_shl), olo = xor_lane<J>(klo, lane, pick_shl);
  const int oi = (int)xor_lane<J>((unsigned)ix, lane, pick_shl);
  const bool take = elem_before(ohi, olo, oi, khi, klo, ix) == keep_better;
  khi = take ? ohi : khi; klo = take ? olo : klo; ix = take ? oi : ix;
}

// ---- The generic kernel: NT threads per utterance (every phase of a frame is a loop over nb * V candidates or over the beam, and one wave per
// SIMD hides neither an LDS nor an L2 latency).  beam_kernel, at the end, is the reference's loop over the phase functions before it. ----
template <int NWV>
struct SelectShared {                            // static LDS of the selection
  double red_v[NWV]; int red_i[NWV + 1];         // arg-max rounds; before them red_i[w] = wave w's number of valid candidates
  unsigned long long wthr[NWV];                  // every wave's bound
  int wcnt[NWV][NWV];                            // ... and how many of wave w's maxima reach wave j's
  int scnt, ovf;                                 // survivors compacted so far | they did not fit the list
};
struct BeamCtx {                                 // what the phases of a frame work on, next to the kernel's arguments `a`
  const BeamArgs &a;
  int tid, lane, wave, b, htmask;
  int nb;                                        // entries of the beam L
  BeamState L, N;                                // this frame's beam and the one it builds
  double *lg, *cand;                             // ln p of the frame | candidate table (LDS or workspace)
  double *dbl; int *ints;                        // the state arrays of GenericLds
  double *sNB, *sB, *sT;                         // this frame's stay / merged entry of every slot
  double *selv, *sv_v; int *sel, *sv_i;          // the selection: candidate and score by rank | survivors of the pruning bound (value | candidate index)
  int *mfrom;                                    // slot that holds the slot's parent labelling (-1: none)
  const double *lm;                              // raw ln-probs (LDS copy or global); lm_scaled() forms the product with alpha per use
  unsigned long long *keys; int *ids, *npar, *nsym;       // trie: hash table, node parents and symbols
  // Lookups instead of scans of the beam:
  //   nslot[node] = beam slot that holds trie node `node` -- written for every entry of a new beam, read by find_parents of the next frame;
  //   cown[c]     = beam slot whose labelling merges with extension candidate c -- written by merge_stays, read by materialise.
  // Neither table is initialised or stamped: a value is USED only if the slot it names passes the very test a scan would apply (L.node[s] ==
  // pnode; mfrom[s] == i && L.last[s] == k), which at most one slot of a beam can pass -- and for a node / candidate that does have such a
  // slot the table was written this frame.  Anything else (stale, never written) fails the test exactly as a scan finds nothing.
  int *nslot, *cown;
  // c / V for candidate indices c < W * V: one multiply-high by ceil(2^32 / V) (exact while c * V < 2^32) -- the runtime division hipcc
  // emits is ~25 instructions, and score_extensions pays it per candidate: the kernel's parallel phases are instruction-issue bound
  unsigned vmagic; bool vmagic_ok;
#ifdef CTCN_BEAM_STATS
  long long gst[16], glast;
#endif
  template <int ORDER>
  __device__ __forceinline__ void carve(unsigned char *lds_base) {
    tid = threadIdx.x; lane = tid & 63; wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (scalar: per-wave decisions are scalar branches)
    b = blockIdx.x; htmask = a.ht_size - 1;
    const int V = a.V, W = a.W, wcap = a.wcap;
    const GenericLds l(V, W, wcap, a.smax, a.cand_in_lds, a.lm_in_lds, ORDER);
    lg = reinterpret_cast<double *>(lds_base);
    cand = a.cand_in_lds ? reinterpret_cast<double *>(lds_base + l.cand) : a.cand_global + (size_t)b * W * V;
    dbl = reinterpret_cast<double *>(lds_base + l.dbl);
    ints = reinterpret_cast<int *>(lds_base + l.ints);
    sNB = dbl + 6 * wcap; sB = sNB + wcap; sT = sB + wcap; selv = sT + wcap; sv_v = selv + wcap;
    mfrom = ints + 8 * wcap; sel = mfrom + wcap; sv_i = sel + wcap;
    lm = a.lm_in_lds ? reinterpret_cast<const double *>(lds_base + l.lm) : a.lm;
    keys = a.ht_keys + (size_t)b * a.ht_size; ids = a.ht_ids + (size_t)b * a.ht_size;
    npar = a.node_par + (size_t)b * a.max_nodes; nsym = a.node_sym + (size_t)b * a.max_nodes;
    nslot = a.node_slot + (size_t)b * a.max_nodes; cown = a.cand_owner + (size_t)b * W * V;
    vmagic = 0xffffffffu / (unsigned)V + 1u;
    vmagic_ok = (unsigned long long)W * V * V < (1ull << 32);          // (a vocabulary of thousands: the plain division)
  }
  template <int ORDER>
  __device__ __forceinline__ BeamState state(int k) const {
    BeamState st;
    st.prev = ORDER == 3 ? sv_i + a.smax + k * a.wcap : nullptr;
    st.pB = dbl + (3 * k) * a.wcap; st.pNB = st.pB + a.wcap; st.pT = st.pNB + a.wcap;
    st.node = ints + (4 * k) * a.wcap; st.len = st.node + a.wcap; st.last = st.len + a.wcap; st.par = st.last + a.wcap;
    return st;
  }
  __device__ __forceinline__ int div_v(int c) const { return vmagic_ok ? (int)__umulhi((unsigned)c, vmagic) : c / a.V; }
};

// 2. which beam slot (if any) holds the parent labelling of slot i' -> its extension by last(i') merges with i'
__device__ __forceinline__ void find_parents(BeamCtx &c) {
  if (c.tid >= c.nb) return;
  const BeamState &L = c.L;
  int m = -1;
  if (L.len[c.tid] > 0) {
    const int pnode = L.par[c.tid];
    if ((unsigned)pnode < (unsigned)c.a.max_nodes) {
      const int sl = c.nslot[pnode];
      if ((unsigned)sl < (unsigned)c.nb && L.node[sl] == pnode) m = sl;
    }
  }
  c.mfrom[c.tid] = m;
}
// 3a. extension scores (calcExtPr) into the candidate table, slot c = i * V + class_col(k).  EU candidates per trip: the slot reads, then the
// LM reads (a round trip to L2 unless the table is in LDS) of all of them are issued before the first is used.
// ORDER 3: the LM term is tri[c0][c1][k] with (c0, c1) = (<s>, <s>) for the empty labelling, (<s>, y[0]) for one class, (y[-2], y[-1]) beyond.
template <int NT, int ORDER>
__device__ __forceinline__ void score_extensions(BeamCtx &c, bool rep_ok) {
  constexpr int EU = 4;
  const BeamState &L = c.L;
  const int V = c.a.V, ncand = c.nb * V;
  for (int c0 = c.tid; c0 < ncand; c0 += EU * NT) {
    int ci[EU], ck[EU], cl[EU], cln[EU];
    double lmv[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int cc = min(c0 + u * NT, ncand - 1);
      ci[u] = c.div_v(cc);
      ck[u] = cand_class(cc - ci[u] * V, c.a.blank);                    // (-1: the stay column)
      cln[u] = L.len[ci[u]]; cl[u] = L.last[ci[u]];
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int c1 = cln[u] > 0 ? cl[u] : V;
      size_t row = (size_t)c1;
      if (ORDER == 3) row += (size_t)(cln[u] > 1 ? L.prev[ci[u]] : V) * (V + 1);
      lmv[u] = c.lm[row * (V + 1) + max(ck[u], 0)];
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int cc = c0 + u * NT;
      if (cc < ncand && ck[u] >= 0) {
        const int i = ci[u], k = ck[u];
        const double bigram = lm_scaled(lmv[u], c.a.alpha);
        const double base = (cln[u] > 0 && cl[u] == k && rep_ok) ? L.pB[i] : L.pT[i];
        c.cand[cc] = c.lg[k] + bigram + base;
      }
    }
  }
}
// 3b. stay entries, merged with the matching extension in the reference's visiting order
__device__ __forceinline__ void merge_stays(BeamCtx &c) {
  if (c.tid >= c.nb) return;
  const BeamState &L = c.L;
  const int ip = c.tid, V = c.a.V;
  double s_nb = LOG_ZERO;
  if (L.len[ip] > 0) s_nb = L.pNB[ip] + c.lg[L.last[ip]];         // BeamSearch.py:102-103
  const double s_b = L.pT[ip] + c.lg[c.a.blank];                    // :106
  Fields e{LOG_ZERO, LOG_ZERO, LOG_ZERO};
  const int i = c.mfrom[ip];
  if (i >= 0) {
    const int ce = i * V + class_col(L.last[ip], c.a.blank);
    c.cown[ce] = ip;
    const double pr = c.cand[ce];
    if (i < ip) { apply_ext(e, pr); apply_stay(e, s_nb, s_b); c.cand[ce] = e.t; c.cand[ip * V] = -INFINITY; }
    else        { apply_stay(e, s_nb, s_b); apply_ext(e, pr); c.cand[ip * V] = e.t; c.cand[ce] = -INFINITY; }
  } else {
    apply_stay(e, s_nb, s_b);
    c.cand[ip * V] = e.t;
  }
  c.sNB[ip] = e.nb; c.sB[ip] = e.b; c.sT[ip] = e.t;
}

// 4. BHat = top-W by (prTotal desc, insertion index asc) without W scans of the table: (a) a lower bound of the W-th best candidate, (b) the
// candidates that reach it into the survivor list, (c) every survivor's rank under cand_better().  Same set and order as W arg-max rounds.
// every thread's candidates, SU loads in flight per thread (a table in global memory would otherwise be a chain of L2 round trips)
template <int NT, typename Visit>
__device__ __forceinline__ void scan_cands(const double *cand, int ncand, int tid, Visit &&visit) {
  constexpr int SU = NT >= 1024 ? 4 : 8;          // (1 024 threads: 128 registers each, and a fourth of the candidates per thread)
  int c = tid;
  for (; c + (SU - 1) * NT < ncand; c += SU * NT) {
    double v[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) v[u] = cand[c + NT * u];
#pragma unroll
    for (int u = 0; u < SU; ++u) visit(v[u], c + NT * u);
  }
  for (; c < ncand; c += NT) visit(cand[c], c);
}
// (a) Every thread keeps the best of its candidates (two with 256 threads); every WAVE finds the k-th largest of its maxima, k = ceil(W /
// waves), by a bitwise search on the keys (ballot + popcount: no LDS, no barrier).  The smallest of the waves' values is always a valid bound
// (waves * k >= W candidates reach it); a larger one is valid whenever W of ALL the maxima reach it, so every wave counts its maxima against
// every wave's value and the largest value with a block-wide count >= W wins.  theta = the bound as a key (0: none), total = valid candidates.
template <int NT>
__device__ __forceinline__ void selection_bound(BeamCtx &c, SelectShared<NT / 64> &ss, int ncand, unsigned long long &theta, int &total) {
  constexpr int NWV = NT / 64;
  constexpr int NH = NT >= 1024 ? 1 : 2;                   // maxima per thread
  const int tid = c.tid, lane = c.lane, wave = c.wave, W = c.a.W;
  unsigned long long tk[NH];
  int nval = 0;
  {
    // the maxima in the double domain (one v_max_f64 per candidate; fmax drops a NaN as "v > -inf" does) and ONE conversion to the key at the
    // end: the scans are instruction-issue bound
    double mx[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) mx[h] = -INFINITY;
    scan_cands<NT>(c.cand, ncand, tid, [&](double v, int cc) {
      nval += v > -INFINITY ? 1 : 0;
      if (NH == 2 && ((cc / NT) & 1)) mx[NH - 1] = fmax(mx[NH - 1], v);
      else mx[0] = fmax(mx[0], v);
    });
#pragma unroll
    for (int h = 0; h < NH; ++h) tk[h] = mx[h] > -INFINITY ? dkey(mx[h]) : 0ull;      // (no candidate: below every key of a finite value)
  }
  GSTAMP(8);
  nval = wave_sum_rows(nval);
  if (lane == 0) ss.red_i[wave] = nval;
  {
    const int kth = (W + NWV - 1) / NWV;
    unsigned long long p = 0ull;
    // two bits per step (the three thresholds of a step are independent ballots), bits 63 .. 36 only: the result is a LOWER bound of the
    // wave's k-th largest maximum either way, 2^-16 relative below it at most, and the search is the most instruction-heavy part of this phase
    for (int bit = 62; bit >= 36; bit -= 2) {
      const unsigned long long t1 = p | (1ull << bit), t2 = p | (2ull << bit), t3 = p | (3ull << bit);
      int c1 = __popcll(__ballot(tk[0] >= t1)), c2 = __popcll(__ballot(tk[0] >= t2)), c3 = __popcll(__ballot(tk[0] >= t3));
      if (NH == 2) {
        c1 += __popcll(__ballot(tk[NH - 1] >= t1)); c2 += __popcll(__ballot(tk[NH - 1] >= t2)); c3 += __popcll(__ballot(tk[NH - 1] >= t3));
      }
      p = c3 >= kth ? t3 : (c2 >= kth ? t2 : (c1 >= kth ? t1 : p));
    }
    if (lane == 0) ss.wthr[wave] = p;
  }
  if (tid == 0) { ss.scnt = 0; ss.ovf = 0; }
  GSTAMP(12);
  __syncthreads();
  GSTAMP(13);
  // lane j keeps wave j's value in registers and v_readlane broadcasts it (no chain of dependent LDS reads); every wave forms the block-wide
  // counts itself from the waves' rows: two barriers, not three
  const unsigned long long tj = ss.wthr[lane < NWV ? lane : 0];
  const int tj_lo = (int)(unsigned)(tj & 0xffffffffull), tj_hi = (int)(unsigned)(tj >> 32);
  int mycnt = 0;
  for (int j = 0; j < NWV; ++j) {
    const unsigned long long t = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(tj_hi, j) << 32) | (unsigned)__builtin_amdgcn_readlane(tj_lo, j);
    int cnt = __popcll(__ballot(tk[0] >= t));
    if (NH == 2) cnt += __popcll(__ballot(tk[NH - 1] >= t));
    mycnt = lane == j ? (t != 0ull ? cnt : 0) : mycnt;
  }
  if (lane < NWV) ss.wcnt[wave][lane] = mycnt;
  GSTAMP(14);
  __syncthreads();
  int reach = 0;
  {
    const int jl = lane < NWV ? lane : 0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) reach += ss.wcnt[w][jl];
    total = lane < NWV ? ss.red_i[jl] : 0;
  }
  theta = (lane < NWV && reach >= W) ? tj : 0ull;
  static_assert(NWV <= 16, "the waves' bounds sit in the first row of 16 lanes");
  total = __builtin_amdgcn_readfirstlane(row16_sum(total));
  theta = row16_max_u64(theta);
  theta = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(theta >> 32)) << 32) |
          (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(theta & 0xffffffffull));
  GSTAMP(9);
}
// (b) the candidates v >= thd into sv_v / sv_i.  One scan: the INDICES of a thread's first two survivors wait in registers, a second scan
// only for a thread with more.  One atomic per WAVE for the position (two ballots; per-thread atomics only with a three-survivor thread).
template <int NT>
__device__ __forceinline__ void compact_survivors(BeamCtx &c, SelectShared<NT / 64> &ss, int ncand, double thd) {
  int cnt = 0, kc0 = 0, kc1 = 0;
  scan_cands<NT>(c.cand, ncand, c.tid, [&](double v, int cc) {
    if (v >= thd) {
      kc0 = cnt == 0 ? cc : kc0;
      kc1 = cnt == 1 ? cc : kc1;
      ++cnt;
    }
  });
  int pos = 0;
  {
    const unsigned long long b1 = __ballot(cnt >= 1), b2 = __ballot(cnt >= 2), b3 = __ballot(cnt >= 3);
    if (b3 == 0ull) {
      const unsigned long long below = (1ull << c.lane) - 1ull;
      const int wtot = __popcll(b1) + __popcll(b2);
      int wbase = 0;
      if (c.lane == 0 && wtot > 0) wbase = atomicAdd(&ss.scnt, wtot);
      pos = __builtin_amdgcn_readfirstlane(wbase) + __popcll(b1 & below) + __popcll(b2 & below);
    } else {
      pos = cnt ? atomicAdd(&ss.scnt, cnt) : 0;
    }
  }
  if (cnt && pos + cnt > c.a.smax) ss.ovf = 1;
  else if (cnt <= 2) {
    if (cnt > 0) { c.sv_v[pos] = c.cand[kc0]; c.sv_i[pos] = kc0; }
    if (cnt > 1) { c.sv_v[pos + 1] = c.cand[kc1]; c.sv_i[pos + 1] = kc1; }
  } else scan_cands<NT>(c.cand, ncand, c.tid, [&](double v, int cc) { if (v >= thd) { c.sv_v[pos] = v; c.sv_i[pos] = cc; ++pos; } });
}
// (c) S <= 256 survivors SORTED, one per thread of waves 0-3, by a bitonic network under the strict order of cand_better() (the padding
// compares equal to itself and worse than every survivor): 36 compare-exchange steps, 33 inside a wave.  Position r of the row IS rank r.
template <int NT>
__device__ __forceinline__ void rank_bitonic(BeamCtx &c, int S) {
  const int tid = c.tid, lane = c.lane;
  unsigned khi = 0u, klo = 0u; int ix = 0x7fffffff;       // (padding: key 0 is below the key of every finite value)
  const bool act = c.wave < 4;                             // (scalar: the other waves only join the barriers of the three cross-wave steps)
  if (act && tid < S) { const unsigned long long k0 = dkey(c.sv_v[tid]); khi = (unsigned)(k0 >> 32); klo = (unsigned)k0; ix = c.sv_i[tid]; }
  const bool pick_shl = (unsigned)__builtin_amdgcn_update_dpp(-1, lane, 0x104, 0xf, 0xf, false) == (unsigned)(lane ^ 4);
  unsigned *const xk = reinterpret_cast<unsigned *>(c.sv_v);     // cross-wave steps: (key hi, key lo) pairs | indices in the survivor arrays
  int *const xi = c.sv_i;
  // element tid of a K-block keeps the better of a pair iff (it is the lower partner) == (its block ends best-first)
#define CTCN_BSTEP(J, K) bitonic_step<J>(khi, klo, ix, ((tid & (J)) == 0) == ((tid & (K)) == 0), lane, pick_shl)
  auto lds_step = [&](int j, int k) {
    if (act) { xk[2 * tid] = khi; xk[2 * tid + 1] = klo; xi[tid] = ix; }
    __syncthreads();
    if (act) {
      const int pt = tid ^ j;
      const unsigned ohi = xk[2 * pt], olo = xk[2 * pt + 1]; const int oi = xi[pt];
      const bool take = elem_before(ohi, olo, oi, khi, klo, ix) == (((tid & j) == 0) == ((tid & k) == 0));
      khi = take ? ohi : khi; klo = take ? olo : klo; ix = take ? oi : ix;
    }
    __syncthreads();
  };
  auto tail = [&](int k) {                           // the in-wave steps j = 32 .. 1 of block size k >= 64
    if (act) { CTCN_BSTEP(32, k); CTCN_BSTEP(16, k); CTCN_BSTEP(8, k); CTCN_BSTEP(4, k); CTCN_BSTEP(2, k); CTCN_BSTEP(1, k); }
  };
  if (act) {
    CTCN_BSTEP(1, 2);
    CTCN_BSTEP(2, 4); CTCN_BSTEP(1, 4);
    CTCN_BSTEP(4, 8); CTCN_BSTEP(2, 8); CTCN_BSTEP(1, 8);
    CTCN_BSTEP(8, 16); CTCN_BSTEP(4, 16); CTCN_BSTEP(2, 16); CTCN_BSTEP(1, 16);
    CTCN_BSTEP(16, 32); CTCN_BSTEP(8, 32); CTCN_BSTEP(4, 32); CTCN_BSTEP(2, 32); CTCN_BSTEP(1, 32);
  }
  tail(64);
  lds_step(64, 128); tail(128);
  lds_step(128, 256); lds_step(64, 256); tail(256);
#undef CTCN_BSTEP
  // (lds_step ends with a barrier: the exchange area is free again; the value is read back from the candidate table, which this path
  // leaves untouched -- bit for bit the double that was scored, where inverting dkey would fold -0.0 onto +0.0)
  if (act && tid < S && tid < c.a.W) { c.sel[tid] = ix; c.selv[tid] = c.cand[ix]; }
}
// (c) any S: a survivor's rank = the survivors that beat it, counted by P neighbouring threads (part p: survivors p, p + P, ...; RU entries
// are read before they are compared: dependent LDS reads cost a full latency each), butterfly sum over the P lanes
template <int NT>
__device__ __forceinline__ void rank_pair_count(BeamCtx &c, int S) {
  const int tid = c.tid;
  int P = 1, lgP = 0;
  while (2 * P * S <= NT && P < 16) { P *= 2; ++lgP; }
  for (int e0 = 0; e0 < S; e0 += NT >> lgP) {
    const int e = e0 + (tid >> lgP), part = tid & (P - 1);
    const bool have = e < S;
    const double mv = c.sv_v[have ? e : 0]; const int mi = c.sv_i[have ? e : 0];
    constexpr int RU = NT >= 1024 ? 4 : 8;
    int rank = 0, q = part;
    for (; q + (RU - 1) * P < S; q += RU * P) {
      double qv[RU]; int qi[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) { qv[u] = c.sv_v[q + u * P]; qi[u] = c.sv_i[q + u * P]; }
#pragma unroll
      for (int u = 0; u < RU; ++u) rank += cand_better(qv[u], qi[u], mv, mi) ? 1 : 0;
    }
    for (; q < S; q += P) rank += cand_better(c.sv_v[q], c.sv_i[q], mv, mi) ? 1 : 0;
    for (int o = 1; o < P; o <<= 1) rank += __shfl_xor(rank, o, 64);
    if (have && part == 0 && rank < c.a.W) { c.sel[rank] = mi; c.selv[rank] = mv; }
  }
}
// the selection: sel[r] / selv[r] = candidate and score of rank r; returns the size of the new beam
template <int NT>
__device__ __forceinline__ int select_top_w(BeamCtx &c, SelectShared<NT / 64> &ss) {
  const int ncand = c.nb * c.a.V, W = c.a.W;
  unsigned long long theta;
  int total;
  selection_bound<NT>(c, ss, ncand, theta, total);
  // (no bound that W maxima reach: then everything valid is ranked, if it fits)
  const bool prune = total > W && theta != 0ull;
  bool ranked = false;
  if (prune || total <= c.a.smax) {
    // The bound as a double: f64_key is an order-preserving bijection of the finite values, so key(v) >= theta <=> v >= thd (one
    // v_cmp_ge_f64; a NaN fails both; theta >= 2^52 > key(-inf) whenever a finite maximum produced it, so "v > -inf" is implied).  Without
    // a bound every finite candidate is ranked: v >= -DBL_MAX.
    const double thd = prune ? key_f64(theta) : -1.7976931348623157e308;
    compact_survivors<NT>(c, ss, ncand, thd);
    __syncthreads();
    GSTAMP(10);
#ifdef CTCN_BEAM_STATS
    if (c.b == 0 && c.tid == 0) { c.gst[6] += ss.scnt; c.gst[7] += ss.ovf ? 1 : 0; }
#endif
    if (!ss.ovf) {
      const int S = ss.scnt;
      if (S <= 256 && c.a.bitonic) rank_bitonic<NT>(c, S);
      else rank_pair_count<NT>(c, S);
      ranked = true;
    }
    __syncthreads();
    GSTAMP(11);
  }
  if (ranked) return min(W, total);
  // (the rounds reuse red_i[], which every thread has just summed into `total`: when the ranking block was skipped no barrier separates those
  // reads from round 0's writes; `ranked` is uniform)
  __syncthreads();
  return arg_max_rounds<NT>(c.cand, ncand, W, ss.red_v, ss.red_i, c.sel, c.selv, c.wave, [] { __syncthreads(); }, [](int) {});
}
// 5. materialise the new beam N: entry r <- candidate sel[r]
template <int ORDER>
__device__ __forceinline__ void materialise(BeamCtx &c, int m, int *s_nodes) {
  if (c.tid >= m) return;
  const BeamState &L = c.L, &N = c.N;
  const int tid = c.tid, cs = c.sel[tid];
  const int i = c.div_v(cs), kk = cs - i * c.a.V;
  auto copy_slot = [&](int s) {
    N.node[tid] = L.node[s]; N.len[tid] = L.len[s]; N.last[tid] = L.last[s]; N.par[tid] = L.par[s];
    N.pNB[tid] = c.sNB[s]; N.pB[tid] = c.sB[s]; N.pT[tid] = c.sT[s];
    if (ORDER == 3) N.prev[tid] = L.prev[s];
  };
  if (kk == 0) {
    copy_slot(i);
  } else {
    const int k = cand_class(kk, c.a.blank);
    int ip = -1;
    {
      const int ow = c.cown[cs];
      if ((unsigned)ow < (unsigned)c.nb && c.mfrom[ow] == i && L.last[ow] == k) ip = ow;
    }
    if (ip >= 0) {   // this slot holds the merged entry of existing labelling ip (first touched as an extension)
      copy_slot(ip);
    } else {
      // trie child lookup / insert: key = (parent node, symbol)
      const int parent = L.node[i];
      const unsigned long long key = ((unsigned long long)(unsigned)parent << 32) | (unsigned)k;
      unsigned h = (unsigned)mix64(key) & c.htmask;
      int id = -1;
      for (int probe = 0; probe <= c.htmask; ++probe) {
        const unsigned long long prev = atomicCAS(&c.keys[h], HT_EMPTY, key);
        if (prev == HT_EMPTY) {
          id = atomicAdd(s_nodes, 1);
          if (id < c.a.max_nodes) { c.npar[id] = parent; c.nsym[id] = k; }
          c.ids[h] = id;
          break;
        }
        if (prev == key) { id = c.ids[h]; break; }
        h = (h + 1) & c.htmask;
      }
      N.node[tid] = id; N.len[tid] = L.len[i] + 1; N.last[tid] = k; N.par[tid] = parent;
      if (ORDER == 3) N.prev[tid] = L.last[i];
      const double pr = c.selv[tid];
      N.pNB[tid] = pr; N.pB[tid] = LOG_ZERO; N.pT[tid] = pr;
    }
  }
  const int nd = N.node[tid];
  if ((unsigned)nd < (unsigned)c.a.max_nodes) c.nslot[nd] = tid;     // (find_parents of the next frame finds a parent labelling's slot here)
}

template <int NT, int ORDER>
__global__ __launch_bounds__(NT) void beam_kernel(BeamArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];   // GenericLds
  __shared__ SelectShared<NT / 64> ss;
  __shared__ int s_flag, s_nodes;
  BeamCtx c = {a};
  c.carve<ORDER>(dsm);
  const int tid = c.tid, lane = c.lane, b = c.b, V = a.V, B = a.B, T = a.T, blank = a.blank;
  if (a.lm_in_lds)                                               // (the raw ln-probs: lm_scaled() rounds the product with alpha on its own per use)
    for (int i = tid; i < (V + 1) * (V + 1); i += NT) const_cast<double *>(c.lm)[i] = a.lm[i];
  int cur = 0, status = 0;
  c.nb = 1;
#ifdef CTCN_BEAM_STATS
  for (int i = 0; i < 16; ++i) c.gst[i] = 0;
  c.glast = clock64();
  long long gframes = 0;
#endif
  if (tid == 0) {
    const BeamState S0 = c.state<ORDER>(0);
    S0.node[0] = 0; S0.len[0] = 0; S0.last[0] = -1; S0.par[0] = -1;
    if (ORDER == 3) S0.prev[0] = -1;
    S0.pB[0] = 0.0; S0.pNB[0] = LOG_ZERO; S0.pT[0] = 0.0;   // BeamSearch.py:83-87
    s_nodes = 1; s_flag = 0;
    c.npar[0] = -1; c.nsym[0] = -1;
    c.nslot[0] = 0;
  }
  __syncthreads();
  const int nframes = min(max(a.lens[b], 0), T);
  // p(blank) of 64 frames per load (lane j: frame chunk0 + j): the skip test of a frame that is not processed costs a register read, not a
  // round trip to memory (peaky posteriors skip two frames of three); the previous frame's value (repeat rule) is carried along
  float pb_lane = 0.0f, pb_before = 0.0f;
  int chunk0 = -64;
  for (int t = 0; t < nframes; ++t) {
    if (t >= chunk0 + 64) {
      chunk0 = t;
      const int tl = min(t + lane, nframes - 1);
      const float *r = a.x + ((size_t)tl * B + b) * V;
      pb_lane = a.input_is_prob ? r[blank] : expf(r[blank]);
    }
    const float pblank = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pb_lane), __builtin_amdgcn_readfirstlane(t - chunk0)));
    const float pprev = pb_before;
    pb_before = pblank;
    if ((1.0f - pblank) < 0.1f) continue;                         // BeamSearch.py:93-94 (float32 compare)
    const bool rep_ok = t > 0 && pprev < 0.9f;                    // BeamSearch.py:63 (float32 compare)
    c.L = c.state<ORDER>(cur); c.N = c.state<ORDER>(cur ^ 1);
    GSTAMP(0);
#ifdef CTCN_BEAM_STATS
    ++gframes;
#endif
    for (int k = tid; k < V; k += NT) {                            // 1. ln of the frame (math.log of the float32 value widened to double)
      const float xk = a.x[((size_t)t * B + b) * V + k], p = a.input_is_prob ? xk : expf(xk);
      if (!(p > 0.0f)) s_flag = 2;
      c.lg[k] = log((double)p);
    }
    find_parents(c);
    __syncthreads();
    if (s_flag == 2) { status = 2; break; }
    GSTAMP(1);
    score_extensions<NT, ORDER>(c, rep_ok);
    __syncthreads();
    GSTAMP(2);
    merge_stays(c);
    __syncthreads();
    GSTAMP(3);
    const int m = select_top_w<NT>(c, ss);
    GSTAMP(4);
    materialise<ORDER>(c, m, &s_nodes);
    __syncthreads();
    GSTAMP(5);
    c.nb = m;
    cur ^= 1;
  }
  __syncthreads();
#ifdef CTCN_BEAM_STATS
  if (a.stats && b == 0 && tid == 0) { for (int i = 0; i < 16; ++i) a.stats[32 + i] = c.gst[i]; a.stats[48] = gframes; }
#endif
  const BeamState L = c.state<ORDER>(cur);
  beam_finish<ORDER>(a, b, status, s_nodes > a.max_nodes, c.nb, L.len, L.last, L.node, L.pT, L.par, c.lm,
                     [&](int &n) { const int sym = c.nsym[n]; n = c.npar[n]; return sym; }, L.prev);
}

// =====================================================================================================================
// Fast path (W <= 60, W*V <= 3328, V <= 256): the same search, restructured around the per-frame latency chain -- the
// double-precision log of the frame, LM gathers from global memory, trie CAS round trips to L2 (~1.9 us each) and chains
// of dependent LDS reads (~100 cycles per hop) of the generic kernel.  Here:
//   * beam_prep_kernel (fully parallel, one wave per (frame, utterance) row) takes everything that does not depend on the
//     beam state out of the chain: ln p as double for every class, p(blank), the "some p is not > 0" flag;
//   * the workgroup compacts its list of processed frames once (the skip rule 1 - p_blank < 0.1 needs no beam state), keeps
//     alpha * LM (31.7 KB at V = 62) in LDS, and every thread prefetches the next frame's ln p of ITS candidate classes;
//   * the beam lives in the registers of wave 0 (lane = beam slot); cross-slot reads are v_readlane / ds_bpermute, not LDS
//     round trips; the per-slot values the candidate scoring needs are mirrored into a small LDS record;
//   * top-W without sorting: waves 3..15 hold the <= W*V candidates (<= 4 per thread); every 16-lane row reduces its largest
//     order-preserving key (high word) on the DPP network, the W-th largest row maximum is a lower bound of the W-th best candidate
//     (exact pruning), the survivors (typically W + a few) are compacted into LDS and ranked by counting with the explicit
//     (score desc, index asc) order of BeamState.sort; more than 256 survivors fall back to block-wide arg-max rounds;
//   * trie: a 16K-slot table IN LDS (node id = slot + 1, entry = {parent id + 1 : 15 | symbol : 17}, double hashing, one ds_cmpst
//     per probe); only when it fills beyond 3/4 do new labellings go to the global-memory table of the generic kernel (64-bit
//     entries {parent : 24 | symbol : 16 | id : 24});
//   * the per-frame serial chain is split over three waves.  Wave 1 owns the trie (a node id is needed a frame later, as
//     the parent id of the labelling's children); wave 0 recognises "this slot's parent labelling was created in this frame" from
//     (grandparent id, parent's last class) keys, which need old ids only.  Wave 2 computes the first level of the stay entries'
//     log-adds (it needs no parent slot) next to wave 0's new-beam work; wave 0 publishes the beam record through an LDS flag, not a
//     barrier.
// Every score is computed by the same expressions on the same operands as in beam_kernel: bit-identical results.  (Against the
// C oracle: identical labellings; float64 scores bit-equal on the golden sets and within 2 ulp elsewhere -- ocml's exp / log vs glibc's.)
// =====================================================================================================================
constexpr int FAST_WMAX = 64;
// a word of the frame list: the frame's number | the repeat rule holds on it (p_blank of the previous frame < 0.9) | one of its p is not > 0
constexpr int FW_ZERO = 1 << 29, FW_REP = 1 << 30, FW_FRAME = FW_ZERO - 1;
// An extension candidate whose labelling is already a beam slot's: mslot[candidate] = {frame tag << MS_TAG_SHIFT | MS_HOLDS |
// slot}.  MS_HOLDS: the candidate holds the slot's merged entry (clear: the entry lives in the slot's stay candidate and this one is
// removed).  selm[] and Survivor::pad carry the low byte, MS_HOLDS | slot, or 0; selm[] = -1 sends decode_sel to mslot[].  TOTS_MASK: a
// survivor's position in tots[].  (Constants only: accessor functions, or cand_class / class_col, in beam_fast_body cost it up to 1.5 %.)
constexpr int MS_HOLDS = 128, MS_SLOT = 63, MS_TAG_SHIFT = 8, TOTS_MASK = 63;

struct FastArgs {
  const double *lgd; const float *pb; const unsigned char *zf;
  const int32_t *lens; const double *lm; double alpha; int W, blank;
  int32_t *out_ids, *out_len; double *out_score; int32_t *status; int T, B, V;
  int nbest; int32_t *out_count;
  unsigned long long *ht; int *node_par; int *node_sym; int ht_size, max_nodes;
  int trie_slots;       // LDS trie slots (power of two)
#ifdef CTCN_BEAM_STATS
  long long *stats;     // development instrumentation (tools/mb_beam.py): cycles per phase of workgroup 0
#endif
};
#ifdef CTCN_BEAM_STATS
#define BSTAMP(i) do { const long long now_ = clock64(); zst[i] += now_ - zlast; zlast = now_; } while (0)
#else
#define BSTAMP(i) do { } while (0)
#endif

__global__ __launch_bounds__(256) void beam_prep_kernel(const float *__restrict__ x, int input_is_prob, double *__restrict__ lgd,
                                                        float *__restrict__ pb, unsigned char *__restrict__ zf, size_t rows, int V, int blank) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *xr = x + row * V;
  bool bad = false;
  for (int k = lane; k < V; k += 64) {
    const float p = input_is_prob ? xr[k] : expf(xr[k]);
    if (!(p > 0.0f)) bad = true;
    lgd[row * V + k] = log((double)p);                 // math.log of the float32 value widened to double
    if (k == blank) pb[row] = p;
  }
  const bool any_bad = __any(bad);
  if (lane == 0) zf[row] = any_bad ? 1 : 0;
}

__device__ __forceinline__ int lane_gather(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }
__device__ __forceinline__ double lane_gather(double v, int src_lane) {
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v)));
}

struct __attribute__((aligned(16))) Survivor { unsigned long long k; int idx; int pad; };
constexpr int SURV_MAX = 256;

constexpr int FAST_NCT = 1024 - 192;                           // candidate threads: waves 3..15
constexpr int FAST_NTH = 1024, FAST_NWV = FAST_NTH / 64;      // 16 waves: the parallel phases are instruction-issue bound (~10 cycles per
                                                               // dependent instruction and wave), so more waves per SIMD is what shortens them
// ORDER 3 (LM_LDS false: the (V+1)^3 table is read from global memory): every slot's record gets the class before the context class
// (bm_c0 beside bm_c1), and wave 0 carries one class more per slot (z_pplast, y[-3]) for the parent's extension term in stay_and_merge.
template <int NPT, bool LM_LDS, int ORDER = 2>
__device__ __forceinline__ void beam_fast_body(FastArgs a) {
  static_assert(ORDER == 2 || (ORDER == 3 && !LM_LDS), "the order-3 table stays in global memory");
  constexpr int NTH = FAST_NTH, NWV = FAST_NWV;
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];   // FastLdsT
  __shared__ Survivor surv[SURV_MAX];                                 // candidates above the pruning bound (order-preserving key, index)
  __shared__ double red_v[NWV];
  __shared__ int red_i[NWV + 1];
  __shared__ unsigned gmax[64];                                        // per 16-lane row: largest candidate key (high word)
  __shared__ double bm_pB[FAST_WMAX], bm_pT[FAST_WMAX], selv[FAST_WMAX];
  __shared__ int selp[FAST_WMAX];                                     // per selected candidate: its position in surv[] (the speculative stay totals are stored by it)
  __shared__ double tots[64];                                         // per survivor: log_add(prBlank', prNonBlank') of the next frame if it is selected (wave 2)
  __shared__ int selm[FAST_WMAX];                                     // per selected candidate: 128 | slot whose merged entry it holds, 0: none, -1: see mslot[]
  __shared__ int bm_c1[2][FAST_WMAX], sel[FAST_WMAX];                 // context class of every slot, by frame parity
  __shared__ int bm_c0[2][ORDER == 3 ? FAST_WMAX : 1], f_c0[ORDER == 3 ? FAST_WMAX : 1];   // order 3: the class before it (V: '<s>') | of the final beam
  __shared__ int f_node[FAST_WMAX], f_len[FAST_WMAX], f_last[FAST_WMAX];   // final beam (dumped once, after the last frame)
  __shared__ double f_pT[FAST_WMAX];
  __shared__ int woff[NWV];
  __shared__ double stayv[FAST_WMAX], homev[FAST_WMAX];
  __shared__ int ns[FAST_WMAX];
  __shared__ double enbv[FAST_WMAX], totv[FAST_WMAX];                // this frame's e.nb of every slot (e.t is homev) | log_add(prBlank', prNonBlank') of the next frame (wave 2)
  __shared__ int nid[2][FAST_WMAX];                                   // node id of every beam slot, double-buffered by frame parity (wave 1)
  __shared__ int s_totflag, s_beamflag, s_decflag;                    // frame number + 1 whose totv[] | beam record (bm_*) | wave 1's decode of the selection is complete
  __shared__ int s_fault;                                             // a bounded wait inside the workgroup ran out (status 4)
  __shared__ int s_cnt;
  __shared__ unsigned s_theta;
  __shared__ int s_nfl, s_gnodes;                // processed frames | 0 while the LDS trie takes inserts, else 1 + global nodes

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, V = a.V, W = a.W, B = a.B, T = a.T, blank = a.blank;
  const int V1 = V + 1;
  const int TS = a.trie_slots;
  const FastLdsT<unsigned> lds(T, V, W, LM_LDS, TS);
  double *lmA = reinterpret_cast<double *>(fsm);
  double *cand = reinterpret_cast<double *>(fsm + lds.cand);
  double *lg2 = reinterpret_cast<double *>(fsm + lds.lg2);
  int *mslot = reinterpret_cast<int *>(fsm + lds.mslot);
  int *flist = reinterpret_cast<int *>(fsm + lds.flist);
  unsigned *trie = reinterpret_cast<unsigned *>(fsm + lds.trie);
  const unsigned tmask = (unsigned)TS - 1u;
  const int tshift = 32 - (31 - __builtin_clz((unsigned)TS));      // top log2(TS) bits of a 32-bit hash
  unsigned long long *ht = a.ht + (size_t)b * a.ht_size;
  int *npar = a.node_par + (size_t)b * a.max_nodes;
  int *nsym = a.node_sym + (size_t)b * a.max_nodes;
  const unsigned htmask = (unsigned)a.ht_size - 1u;

  if (LM_LDS)
    for (int i = tid; i < V1 * V1; i += NTH) lmA[i] = a.lm[i] * a.alpha;        // rounded by the store: the same product lm_scaled() gives the generic kernel and the global-memory variant per use
  for (int i = tid; i < W * V; i += NTH) mslot[i] = -1;
  for (int i = tid; i < TS; i += NTH) trie[i] = 0u;
  const int nframes = min(max(a.lens[b], 0), T);
  if (tid == 0) {
    bm_c1[0][0] = V; bm_pB[0] = 0.0; bm_pT[0] = 0.0;                             // the empty labelling: prBlank = prTotal = 0 (BeamSearch.py:83-87)
    if (ORDER == 3) bm_c0[0][0] = V;
    s_nfl = 0; s_gnodes = 0; s_totflag = 0; s_beamflag = 0; s_decflag = 0; s_fault = 0;
  }
  if (tid < 64) gmax[tid] = 0u;                                                  // (rows 52..63 belong to no candidate wave: they stay 0)
  if (tid < 2 * FAST_WMAX) nid[0][tid] = 0;                                       // (both parities: node 0 = the empty labelling)
  __syncthreads();
  // frames the search processes, in order (BeamSearch.py:93-94: skip when 1 - p_blank < 0.1, a float32 compare), each with its
  // "p_blank of the previous frame < 0.9" bit (:63) and its "log(0)" bit
  for (int t0 = 0; t0 < nframes; t0 += NTH) {
    const int t = t0 + tid;
    bool keep = false;
    int word = 0;
    if (t < nframes) {
      const float pbl = a.pb[(size_t)t * B + b];
      keep = !((1.0f - pbl) < 0.1f);
      const bool rep = t > 0 && a.pb[(size_t)(t - 1) * B + b] < 0.9f;
      word = t | (rep ? FW_REP : 0) | (a.zf[(size_t)t * B + b] ? FW_ZERO : 0);
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) woff[wave] = __popcll(mask);
    __syncthreads();
    int base = s_nfl;
    for (int w = 0; w < wave; ++w) base += woff[w];
    if (keep) flist[base + __popcll(mask & ((1ull << lane) - 1ull))] = word;
    __syncthreads();
    if (tid == 0) { int add = 0; for (int w = 0; w < NWV; ++w) add += woff[w]; s_nfl += add; }
    __syncthreads();
  }
  const int nfl = s_nfl;

  // Wave 0 owns the beam (lane = slot) and the serial chain, wave 1 the prefix trie (node ids are only needed a frame later), wave 2 the
  // log-add of every slot's stay entry that needs no parent slot; waves 3..15 (832 threads) own the candidates.
  // That log-add -- exp and log in f64, ~1.8 k cycles of one wave -- is the longest link of the frame.  Wave 2 forms it for every SURVIVOR of
  // the pruning bound (at most 64, one per lane) while the candidate waves still rank them: up to 1 + exp(.) before the barrier that ends the
  // rank count, the logarithm behind it; wave 0 picks the totals of the selected survivors up by their position (selp[] -> tots[]).  With
  // more than 64 survivors the total is formed behind the decode of the selection (totv[]).  The split point is where it is because the
  // barrier must not wait for wave 2 (DESIGN_HISTORY.md, "decode.hip: tried and not kept").
  // Every role runs ITS OWN frame loop below (same barriers, in the same order): the kernel sits at its register limit, and with the roles
  // interleaved phase by phase in one loop every role's state was live everywhere -- the allocator spilled loop-invariant addresses to
  // scratch and re-loaded them inside the frame's critical path.  In separate branches the live ranges do not overlap.
  constexpr int NCT = FAST_NCT;
  // ln p row of the next frame, one frame ahead, held by threads 128 .. 128 + V - 1 (waves 2..5: wave 0's instruction stream is the
  // critical chain); lg[p] = row of the frames of parity p, written at the top of the frame BEFORE the one that uses it, so that every
  // reader finds it behind the selection's barriers
  double nlg = 0.0;
  const int lgk = tid - 128;
  auto fetch_lg = [&](int fword) {
    if (lgk >= 0 && lgk < V) nlg = a.lgd[((size_t)(fword & FW_FRAME) * B + b) * V + lgk];
  };
  if (nfl > 0) fetch_lg(flist[0]);
  if (lgk >= 0 && lgk < V) lg2[lgk] = nlg;
  if (nfl > 1) fetch_lg(flist[1]);
  auto frame_top = [&](int j) {                                  // (holders only) the next frame's ln p row: its last readers were frame j - 1's
    if (lgk >= 0 && lgk < V && j + 1 < nfl) lg2[((j + 1) & 1) * V + lgk] = nlg;
    if (j + 2 < nfl) fetch_lg(flist[j + 2]);
  };
  int nb = 1, status = 0;
  // the serial chain (wave 0) and its two helpers win the issue arbitration of their SIMDs against the scoring waves they share them with (0.3-0.9 %)
  if (wave == 0) __builtin_amdgcn_s_setprio(3); else if (wave == 2) __builtin_amdgcn_s_setprio(2); else if (wave == 1) __builtin_amdgcn_s_setprio(1);
  // The pruning bound is formed in the selection, behind the scoring phase, not inside it: the parallel phases are issue-bound, and extra
  // instructions in thirteen waves end up behind wave 0's chain (DESIGN_HISTORY.md, "decode.hip: tried and not kept").
  __syncthreads();
#ifdef CTCN_BEAM_STATS
  long long zst[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, zlast = clock64(), zrounds = 0, ziters = 0;
  const long long zt0 = zlast;
#endif
  // more than SURV_MAX candidates above the bound (exact ties: synth's ties16 at W = 52; never on the benchmark's regimes): W block-wide arg-max rounds over the candidate
  // table (wave 0 patches it first so that it holds this frame's stay / merged entries), exactly as the generic kernel does.  All threads.
  auto rounds = [&]() -> int {
#ifdef CTCN_BEAM_STATS
    ++zrounds;
#endif
    return arg_max_rounds<NTH>(cand, nb * V, W, red_v, red_i, sel, selv, wave, [] { lds_barrier(); }, [&](int r) { selm[r] = -1; });
  };
  // waves 0..2: decode of the selection -- new slot `lane` <- candidate sel[lane]: which old slot it comes from, fresh labelling or copy
  struct Dec { bool act, fresh; int src, sym; double sv; };
  auto decode_sel = [&](int j, int m) -> Dec {
    Dec d;
    const int rr = min(lane, FAST_WMAX - 1);
    const int c = sel[rr];
    d.sv = selv[rr];
    d.act = lane < m;
    const int i = d.act ? (int)(((float)c + 0.5f) * (1.0f / (float)V)) : 0;       // c / V (exact for c < 2^20)
    const int kk = c - i * V;
    d.sym = (kk - 1 < blank) ? kk - 1 : kk;
    // does this candidate hold the merged entry of a slot?  The candidate's thread looked that up when it loaded the value (selm[]: one LDS
    // round trip less on the serial chain); -1: the selection came from the arg-max rounds, mslot[] has it
    int sm = selm[rr];
    if (sm < 0) { const int ms = mslot[d.act ? c : 0]; sm = (kk != 0 && ms >= 0 && (ms >> MS_TAG_SHIFT) == j && (ms & MS_HOLDS)) ? (MS_HOLDS | (ms & MS_SLOT)) : 0; }
    const bool merged = d.act && (sm & MS_HOLDS);
    d.fresh = d.act && kk != 0 && !merged;
    d.src = merged ? (sm & MS_SLOT) : i;
    return d;
  };
  const bool first_ok = nfl > 0 && !(flist[0] & FW_ZERO);
  const bool rep0 = nfl > 0 && (flist[0] & FW_REP) != 0;

  if (wave >= 3) {
    // ======================================= waves 3..15: the candidates =======================================================
    // slot i of thread u = tid - 192 is c = ((37 * u) mod 832) + 832 * i -> (beam ci, class ck; ck < 0: the stay slot).  Any bijection works
    // (the selection ranks by explicit (score, index)); the multiplier spreads neighbouring candidates -- the classes of one beam -- over
    // different 16-lane rows, which keeps the pruning bound of the selection tight.
    const int u = tid - 192;
    int cc[NPT], ci[NPT], ck[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int c = ((37 * u) % NCT) + i * NCT;
      cc[i] = min(c, W * V - 1);
      ci[i] = c < W * V ? c / V : FAST_WMAX;                      // beyond the table: never valid (nb <= W <= FAST_WMAX)
      const int kk = c - (c / V) * V;
      ck[i] = kk == 0 ? -1 : ((kk - 1 < blank) ? kk - 1 : kk);
    }
    // extension scores (calcExtPr) of frame jf into cand[]: two LDS hops (the slot's context class, then LM / prBlank / prTotal), every
    // read of a hop issued before the first use (clamped addresses, selects afterwards)
    auto score_extensions = [&](bool rep_ok, int jf) {
      const double *lg = lg2 + (jf & 1) * V;
      int c1[NPT], c0[NPT];
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        c1[i] = bm_c1[jf & 1][min(ci[i], FAST_WMAX - 1)];
        c0[i] = ORDER == 3 ? bm_c0[jf & 1][min(ci[i], FAST_WMAX - 1)] : 0;
      }
      double lmv[NPT], pbv[NPT], ptv[NPT], lk[NPT];
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        const int bi = min(ci[i], FAST_WMAX - 1), k = max(ck[i], 0);
        const int c1c = min(max(c1[i], 0), V);
        size_t row = (size_t)c1c;
        if (ORDER == 3) row += (size_t)min(max(c0[i], 0), V) * V1;
        lmv[i] = LM_LDS ? lmA[c1c * V1 + k] : lm_scaled(a.lm[row * V1 + k], a.alpha);
        lk[i] = lg[k];
        pbv[i] = bm_pB[bi];
        ptv[i] = bm_pT[bi];
      }
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        if (ci[i] < nb && ck[i] >= 0) {
          const double base = (c1[i] == ck[i] && rep_ok) ? pbv[i] : ptv[i];     // c1 == k <=> non-empty labelling ending in k
          cand[cc[i]] = lk[i] + lmv[i] + base;
        }
      }
    };
    if (first_ok) score_extensions(rep0, 0);
    lds_barrier();
    for (int j = 0, fw = nfl > 0 ? flist[0] : 0; j < nfl; ++j) {  // (fw: the frame's word, read one frame ahead)
      if (fw & FW_ZERO) { status = 2; break; }                   // math.log(0) in the reference: ValueError
      frame_top(j);
      BSTAMP(0);
      // P3: BHat = top-W by (prTotal desc, candidate index asc), without sorting.
      //  1. splitter: every 16-lane row reduces the largest key (high word) of its 16 * NPT candidates on the DPP network; the W-th largest
      //     of the 52 row maxima is a lower bound of the W-th best candidate (W distinct candidates reach it): exact pruning;
      //  2. the survivors (typically W + a few) are compacted into LDS and ranked by counting, the candidate threads sharing the compares.
      unsigned long long key[NPT];
      bool val[NPT];
      unsigned mhi = 0u, mpack = 0u;                                // mpack: byte i = MS_HOLDS | slot when candidate i holds that slot's merged entry
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        const int bi = min(ci[i], FAST_WMAX - 1);
        double v = ck[i] < 0 ? stayv[bi] : cand[cc[i]];
        const int ms = mslot[cc[i]];
        if (ck[i] >= 0 && ms >= 0 && (ms >> MS_TAG_SHIFT) == j) {
          v = (ms & MS_HOLDS) ? homev[ms & MS_SLOT] : -INFINITY;
          if (ms & MS_HOLDS) mpack |= (unsigned)(MS_HOLDS | (ms & MS_SLOT)) << (8 * i);
        }
        key[i] = f64_key(v);
        val[i] = ci[i] < nb && v != -INFINITY;
        mhi = max(mhi, val[i] ? (unsigned)(key[i] >> 32) : 0u);
      }
      mhi = row16_umax(mhi);
      if ((lane & 15) == 15) gmax[u >> 4] = mhi;
      BSTAMP(8);
      lds_barrier();
      {
        // rank of row maximum e among the 52 (ties broken by the row number: a strict order); 16 threads per row maximum (gmax[52..63] stay 0)
        const int e = u >> 4, part = u & 15;
        const unsigned mine = gmax[e];
        int cnt = 0;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int q = part * 4 + q4;
          const unsigned o = gmax[q];
          cnt += (o > mine || (o == mine && q < e)) ? 1 : 0;
        }
        cnt = row16_sum(cnt);
        if (part == 0 && cnt == W - 1) s_theta = mine;                        // (no such row when fewer than W rows hold a candidate: 0)
      }
      lds_barrier();
      {
        const unsigned theta = s_theta;
        bool keep[NPT];
        int wtot = 0, pos[NPT];
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
          keep[i] = val[i] && (unsigned)(key[i] >> 32) >= theta;
          const unsigned long long bal = __ballot(keep[i]);
          pos[i] = wtot + __popcll(bal & ((1ull << lane) - 1ull));
          wtot += __popcll(bal);
        }
        int wbase = 0;
        if (lane == 0 && wtot > 0) wbase = atomicAdd(&s_cnt, wtot);
        wbase = __builtin_amdgcn_readfirstlane(wbase);
#pragma unroll
        for (int i = 0; i < NPT; ++i)
          if (keep[i] && wbase + pos[i] < SURV_MAX) {
            Survivor sv;
            sv.k = key[i]; sv.idx = ci[i] * V + (ck[i] < 0 ? 0 : (ck[i] < blank ? ck[i] + 1 : ck[i])); sv.pad = (int)((mpack >> (8 * i)) & 255u);
            surv[wbase + pos[i]] = sv;
          }
      }
      BSTAMP(3);
      lds_barrier();
      // (the reads of the common case -- up to 52 survivors, 16 threads each -- are issued before the survivor count is known: one LDS round trip
      // instead of three in a row)
      // (thread index of the rank count: the candidate waves that share wave 2's SIMD -- 6, 10, 14 -- take the last survivors, which rarely
      // exist, so that wave 2's log-add has that SIMD to itself)
      const int cw = wave - 3;
      const int ur = (((cw & 3) == 3) ? 10 + (cw >> 2) : cw - (cw >> 2)) * 64 + lane;
      const Survivor me16 = surv[ur >> 4];
      Survivor oe16[4];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) oe16[q4] = surv[(ur & 15) + 16 * q4];
      const int S = s_cnt;
      int total = S;
      if (S <= 52) {
        if ((ur & ~63) < S * 16) {
          const int e = ur >> 4, part = ur & 15;
          int cnt = 0;
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4)
            cnt += (part + 16 * q4 < S && (oe16[q4].k > me16.k || (oe16[q4].k == me16.k && oe16[q4].idx < me16.idx))) ? 1 : 0;
          cnt = row16_sum(cnt);
          if (e < S && part == 0 && cnt < W) { sel[cnt] = me16.idx; selv[cnt] = key_f64(me16.k); selm[cnt] = me16.pad; selp[cnt] = e; }
        }
      } else if (S <= SURV_MAX) {
        // rank counting: P of the 832 candidate threads per survivor, thread part p compares it with survivors p, p + P, ...; DPP butterfly sum
        const int P = S <= 104 ? 8 : (S <= 208 ? 4 : 2);
        if ((ur & ~63) < S * P) {                                 // (waves whose 64 / P survivors do not exist go straight to the barrier: the
                                                                 // phase is issue-bound, fewer waves per SIMD finish it sooner)
          const int e = ur / P, part = ur - e * P;
          const Survivor me = surv[min(e, SURV_MAX - 1)];
          int cnt = 0;
          for (int q0 = part; q0 < S; q0 += 4 * P) {
            Survivor oe[4];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) oe[q4] = surv[min(q0 + q4 * P, SURV_MAX - 1)];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
              cnt += (q0 + q4 * P < S && (oe[q4].k > me.k || (oe[q4].k == me.k && oe[q4].idx < me.idx))) ? 1 : 0;
          }
          cnt += __builtin_amdgcn_update_dpp(0, cnt, 0xB1, 0xf, 0xf, true);                  // quad_perm [1,0,3,2]
          if (P >= 4) cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
          if (P >= 8) cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x141, 0xf, 0xf, true);     // row_half_mirror
          if (e < S && part == 0 && cnt < W) { sel[cnt] = me.idx; selv[cnt] = key_f64(me.k); selm[cnt] = me.pad; selp[cnt] = e; }
        }
      } else {
        lds_barrier();                                             // (wave 0 has patched the candidate table)
        total = rounds();
      }
      lds_barrier();
      BSTAMP(4);
      nb = min(W, total);
      const int fwn = flist[min(j + 1, nfl - 1)];
      const bool more = j + 1 < nfl && !(fwn & FW_ZERO);
      if (more) {
        // the new beam's record (context class, prBlank, prTotal of every slot) comes from wave 0 through a flag, not a barrier
        for (int spins = 0; __hip_atomic_load(&s_beamflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != j + 1; ++spins) {
          if (spins > (1 << 20)) { s_fault = 1; break; }
          __builtin_amdgcn_s_sleep(2);
        }
        BSTAMP(6);
        score_extensions((fwn & FW_REP) != 0, j + 1);
        BSTAMP(9);
      }
      fw = fwn;
      lds_barrier();
      BSTAMP(2);
    }
  } else if (wave == 0) {
    // ======================================= wave 0: the beam and the serial chain =============================================
    // lane r holds slot r.  node ids: 0 = the empty labelling, s + 1 = LDS trie slot s, TS + 1 + g = entry g of the global table.
    // z_mf = the slot that holds this slot's parent labelling (-1: none) -- its extension by z_last IS this labelling.
    // Wave 0 never waits for the trie: the id of a slot's OWN labelling lives with wave 1 (handed over through nid[] a frame later, when
    // a child needs it as its z_par).  What wave 0 carries instead is the parent labelling's key, (z_gpar, z_plast) = (id of the
    // grandparent labelling, last class of the parent labelling): a labelling created in this frame as (parent id p, class k) IS the
    // parent of slot r exactly when p == z_gpar[r] and k == z_plast[r] (ids are unique per (parent, class)), which needs old ids only.
    int z_len = 0, z_last = -1, z_par = -1, z_mf = -1, z_gpar = -2, z_plast = -1;
    int z_pplast = -1;                                             // order 3: the class before z_plast (y[-3])
    double z_pB = 0.0, z_pNB = LOG_ZERO, z_pT = 0.0;
    double e_nb = LOG_ZERO, e_b = LOG_ZERO, e_t = LOG_ZERO;        // this frame's stay / merged entry of the slot (BeamSearch.py:99-113)
    // stay entries of every slot, merged with the extension of the parent slot that equals the labelling (same expression, same operands
    // as score_extensions writes for that candidate).  Results: e_nb / e_b / e_t in the slot's lane; for the selection: stayv[ip] = value
    // of the stay candidate (or -inf when the entry lives in the extension's place), homev[ip] = e_t, and mslot[extension candidate] =
    // {frame tag, 1: holds slot ip's merged entry | 0: removed (merged into the stay candidate), ip}
    auto stay_and_merge = [&](bool rep_ok, int jf, int tsrc) {
      const int ip = lane;
      const double *lg = lg2 + (jf & 1) * V;
      const double lgl = lg[max(z_last, 0)], lgb = lg[blank];
      const int mi = ip < nb ? z_mf : -1;
      const int src = max(mi, 0);
      const double p_pB = lane_gather(z_pB, src), p_pT = lane_gather(z_pT, src);
      // (context class of the parent labelling: its last class travels with the slot -- z_plast -- and its length is this one's minus one:
      // the LM term is read next to the ln p terms, not behind the parent slot)
      const int c1 = z_len > 1 ? max(z_plast, 0) : V, k = max(z_last, 0);
      size_t row = (size_t)c1;
      if (ORDER == 3) row += (size_t)(z_len > 2 ? max(z_pplast, 0) : V) * V1;
      const double lmv = LM_LDS ? lmA[c1 * V1 + k] : lm_scaled(a.lm[row * V1 + k], a.alpha);
      const double base = (c1 == k && rep_ok) ? p_pB : p_pT;
      const double pr = lgl + lmv + base;                           // == cand[mi * V + kk(z_last)]
      double s_nb = LOG_ZERO;
      if (z_len > 0) s_nb = z_pNB + lgl;                            // BeamSearch.py:102-103
      const double s_b = z_pT + lgb;                                // :106
      const bool ext_first = mi >= 0 && mi < ip;                    // the reference meets the extension before the stay entry
      BSTAMP(6);
      // tot = log_add(s_b, s_nb) of every slot comes from wave 2 (it needs no parent slot, so it is computed next to the lines above)
      // (bounded: wave 2 reaches its store whenever this wave gets here -- both follow the wave-uniform `more` -- so the bound only turns a
      // programming error into status 4 instead of a hung workgroup)
      // -- and mslot[] below is rewritten only once wave 1, too, has decoded this frame's selection (s_decflag; set thousands of cycles ago)
      for (int spins = 0; __hip_atomic_load(&s_totflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != jf + 1 ||
                          __hip_atomic_load(&s_decflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != jf; ++spins) {
        if (spins > (1 << 20)) { s_fault = 1; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      const double tot = tsrc >= 0 ? tots[tsrc] : totv[ip];
      double r_nb = s_nb, r_t = tot;
      if (__any(mi >= 0)) {                                          // some slot merges with its parent's extension: ONE level of log-adds
        // lanes 0..31: e.t of slot q, lanes 32..63: e.nb of slot q, q = (lane & 31) + 32 * pass -- side by side (one pass when nb <= 32)
#pragma nounroll
        for (int q0 = 0; q0 < nb; q0 += 32) {
          const int q = (lane & 31) + q0;
          const double q_snb = lane_gather(s_nb, q), q_pr = lane_gather(pr, q), q_tot = lane_gather(tot, q);
          const int q_mi = lane_gather(mi, q);
          const bool q_first = q_mi >= 0 && q_mi < q;
          const double other = lane < 32 ? q_tot : q_snb;
          const double ax = q_first ? q_pr : other, ay = q_first ? other : q_pr;      // the reference's argument order (extension met first or second)
          const double r1 = q_mi >= 0 ? log_add_prob(ax, ay) : LOG_ZERO;
          const int from = (lane & 31);                              // slot ip = q0 + from reads lanes from (e.t) and from + 32 (e.nb)
          const double a_t = lane_gather(r1, from), a_nb = lane_gather(r1, from + 32);
          if (mi >= 0 && (ip >> 5) == (q0 >> 5)) { r_nb = a_nb; r_t = a_t; }
        }
      }
      BSTAMP(7);
      if (ip < nb) {
        e_nb = r_nb; e_b = s_b; e_t = r_t;
        homev[ip] = r_t; enbv[ip] = r_nb;
        stayv[ip] = ext_first ? -INFINITY : r_t;
        if (mi >= 0) mslot[mi * V + ((z_last < blank) ? z_last + 1 : z_last)] = (jf << MS_TAG_SHIFT) | (ext_first ? MS_HOLDS : 0) | ip;
      }
      if (lane == 0) { s_theta = 0u; s_cnt = 0; }
    };
    if (first_ok) stay_and_merge(rep0, 0, -1);
    lds_barrier();
    for (int j = 0, fw = nfl > 0 ? flist[0] : 0; j < nfl; ++j) {
      if (fw & FW_ZERO) { status = 2; break; }
      BSTAMP(0);
      lds_barrier();                                               // (row maxima)
      lds_barrier();                                               // (pruning bound)
      BSTAMP(3);
      lds_barrier();                                               // (survivors compacted)
      const int S = s_cnt;
      int total = S;
      if (S > SURV_MAX) {
        if (lane < nb) {
          cand[lane * V] = stayv[lane];
          if (z_mf >= 0) cand[z_mf * V + ((z_last < blank) ? z_last + 1 : z_last)] = (z_mf < lane) ? homev[lane] : -INFINITY;
        }
        lds_barrier();
        total = rounds();
      }
      lds_barrier();                                               // (selection ranked)
      BSTAMP(4);
      const int m = min(W, total);
      const int fwn = flist[min(j + 1, nfl - 1)];
      const bool more = j + 1 < nfl && !(fwn & FW_ZERO);
      const bool rep_next = (fwn & FW_REP) != 0;
      // P4a: the new beam in rank order; the record the next frame's extension scores need goes out through s_beamflag (wave 0 does not stop)
      const Dec d = decode_sel(j, m);
      const int tsrc = (more && S <= 64) ? (selp[min(lane, FAST_WMAX - 1)] & TOTS_MASK) : -1;   // where wave 2 leaves this slot's stay total (tots[]; -1: totv[])
      const bool act = d.act, fresh = d.fresh;
      const int src = d.src, sym = d.sym;
      ns[lane] = -1;
      const int g_len = lane_gather(z_len, src), g_last = lane_gather(z_last, src), g_par = lane_gather(z_par, src);
      const int g_gpar = lane_gather(z_gpar, src), g_plast = lane_gather(z_plast, src);
      const int g_pplast = ORDER == 3 ? lane_gather(z_pplast, src) : -1;
      const int g_nid = nid[j & 1][src];                           // id of the old slot's labelling (wave 1, previous frame)
      const int g_mf = lane_gather(z_mf, src);
      const double g_nb = lane_gather(e_nb, src), g_b = lane_gather(e_b, src), g_t = lane_gather(e_t, src);
      int n_len = g_len, n_last = g_last, n_par = g_par, n_gpar = g_gpar, n_plast = g_plast, n_mf = -1;
      int n_pplast = g_pplast;
      double n_pNB = g_nb, n_pB = g_b, n_pT = g_t;
      if (fresh) {
        n_len = g_len + 1; n_last = sym; n_par = g_nid; n_gpar = g_len > 0 ? g_par : -2; n_plast = g_last;
        n_pplast = g_plast;
        n_pNB = d.sv; n_pB = LOG_ZERO; n_pT = d.sv;
      }
      if (act) { bm_c1[(j + 1) & 1][lane] = n_len > 0 ? n_last : V; bm_pB[lane] = n_pB; bm_pT[lane] = n_pT; }
      if (ORDER == 3 && act) bm_c0[(j + 1) & 1][lane] = n_len > 1 ? n_plast : V;
      if (act && !fresh) ns[src] = lane;                           // where the old slot's labelling went
      __hip_atomic_store(&s_beamflag, j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      BSTAMP(5);
      nb = m;
      // P4b: parent slot of every new slot, then the stay / merge entries of the NEXT frame.  A fresh labelling's parent is the old slot it
      // extends; a copy's parent is the old slot's parent, wherever that went -- or, when the parent was NOT in the old beam, possibly a
      // labelling created just now: fresh lane f holds labelling (parent id n_par[f], class n_last[f]), which is slot r's parent exactly
      // when that pair equals (n_gpar[r], n_plast[r]).  The loop walks the shorter of the two lane sets.
      {
        const int pm = fresh ? src : g_mf;
        n_mf = (act && pm >= 0 && n_len > 0) ? ns[pm] : -1;
        const bool scan = act && !fresh && n_len > 1 && g_mf < 0;   // (a labelling of length 1 has the empty labelling as parent: never fresh)
        unsigned long long fmask = __ballot(fresh), smask = __ballot(scan);
        if (smask != 0ull && fmask != 0ull) {
          if (__popcll(fmask) <= __popcll(smask)) {
            while (fmask) {
              const int fl = __ffsll((long long)fmask) - 1;
              fmask &= fmask - 1;
              const int fp = __builtin_amdgcn_readlane(n_par, fl), fk = __builtin_amdgcn_readlane(n_last, fl);
              if (scan && fp == n_gpar && fk == n_plast) n_mf = fl;
            }
          } else {
            while (smask) {
              const int sl = __ffsll((long long)smask) - 1;
              smask &= smask - 1;
              const int gp = __builtin_amdgcn_readlane(n_gpar, sl), pk = __builtin_amdgcn_readlane(n_plast, sl);
              const unsigned long long hit = __ballot(fresh && n_par == gp && n_last == pk);
              if (hit != 0ull && lane == sl) n_mf = __ffsll((long long)hit) - 1;
            }
          }
        }
      }
      z_len = n_len; z_last = n_last; z_par = n_par; z_gpar = n_gpar; z_plast = n_plast; z_mf = n_mf; z_pNB = n_pNB; z_pB = n_pB; z_pT = n_pT;
      if (ORDER == 3) z_pplast = n_pplast;
      if (more) stay_and_merge(rep_next, j + 1, tsrc);
      fw = fwn;
      lds_barrier();
      BSTAMP(2);
    }
    f_len[lane] = z_len; f_last[lane] = z_last; f_pT[lane] = z_pT;
    if (ORDER == 3 && lane < FAST_WMAX) f_c0[lane] = z_plast;
  } else {
    // ======================================= waves 1 and 2: the trie | the stay totals ==========================================
    int y_node = 0, y_lnodes = 0;                                  // wave 1: node id of slot `lane`; LDS trie nodes so far (wave-uniform)
    // wave 2: tot = log_add(prBlank', prNonBlank') (BeamSearch.py:112) of the stay entry of every slot for frame jf, from the slot's (context
    // class, prNonBlank, prTotal) -- the same expressions on the same operands as wave 0 forms for s_nb / s_b -- then the flag wave 0 waits
    // for.  It needs no parent slot, so it runs next to wave 0's new-beam / parent-slot work instead of in front of its log-add
    auto stay_total = [&](int jf, bool on, int c1, double pNB, double pT) -> double {
      const double *lg = lg2 + (jf & 1) * V;
      const double lgl = lg[c1 < V ? c1 : 0], lgb = lg[blank];
      double s_nb = LOG_ZERO;
      if (c1 < V) s_nb = pNB + lgl;
      const double s_b = pT + lgb;
      return on ? log_add_prob(s_b, s_nb) : LOG_ZERO;
    };
    auto stay_totals = [&](int jf, bool on, int c1, double pNB, double pT) {
      totv[lane] = stay_total(jf, on, c1, pNB, pT);
      __hip_atomic_store(&s_totflag, jf + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    if (first_ok && wave == 2) stay_totals(0, lane == 0, V, LOG_ZERO, 0.0);       // the empty labelling
    lds_barrier();
    for (int j = 0, fw = nfl > 0 ? flist[0] : 0; j < nfl; ++j) {
      if (fw & FW_ZERO) { status = 2; break; }
      frame_top(j);
      BSTAMP(0);
      lds_barrier();
      lds_barrier();
      lds_barrier();
      const int S = s_cnt;
      int total = S;
      const int fwn = flist[min(j + 1, nfl - 1)];
      const bool more = j + 1 < nfl && !(fwn & FW_ZERO);
      // wave 2, while the candidate waves rank the survivors: the next frame's stay total of EVERY survivor (at most 64: one per lane), from
      // what its new slot would carry -- a fresh labelling its candidate's score, a copy the stay / merged entry of the slot it comes from --
      // so that the log-add is over when wave 0 asks for it, instead of starting behind the decode of the selection
      const bool spec = wave == 2 && more && S <= 64;
      double sp_x = LOG_ZERO, sp_s = 1.0;
      bool sp_half = false;
      if (spec) {
        const Survivor sv = surv[lane];
        const bool on = lane < S;
        const int c = on ? sv.idx : 0;
        const int i = (int)(((float)c + 0.5f) * (1.0f / (float)V));
        const int kk = c - i * V;
        const int sym = (kk - 1 < blank) ? kk - 1 : kk;
        const bool merged = on && (sv.pad & MS_HOLDS);
        const bool fresh = on && kk != 0 && !merged;
        const int src = merged ? (sv.pad & MS_SLOT) : i;
        const double v = key_f64(sv.k);
        const int o_c1 = bm_c1[j & 1][src];
        const double o_nb = enbv[src], o_t = homev[src];
        // log_add_prob(prBlank', prNonBlank') in two halves: up to 1 + exp(.) before the barrier the candidate waves' rank count ends with, the
        // logarithm behind it (the whole chain, ~1.8 k cycles, would hold that barrier up; the store keeps the first half on this side of it)
        const int c1 = fresh ? sym : o_c1;
        const double pNB = fresh ? v : o_nb, pT = fresh ? v : o_t;
        const double *lg = lg2 + ((j + 1) & 1) * V;
        const double lgl = lg[c1 < V ? c1 : 0], lgb = lg[blank];
        const double s_nb = c1 < V ? pNB + lgl : LOG_ZERO, s_b = pT + lgb;
        sp_half = false;
        if (!on) sp_x = LOG_ZERO;
        else if (s_b <= LOG_ZERO) sp_x = s_nb;
        else if (s_nb <= LOG_ZERO) sp_x = s_b;
        else {
          double x = s_b, y = s_nb;
          if ((y - x) > 0.0) { x = s_nb; y = s_b; }
          sp_x = x; sp_s = 1 + exp(y - x); sp_half = true;
        }
        tots[lane] = sp_s;
      }
      if (S > SURV_MAX) { lds_barrier(); total = rounds(); }
      lds_barrier();
      BSTAMP(4);
      const int m = min(W, total);
      Dec d = {false, false, 0, 0, 0.0};
      if (!spec) d = decode_sel(j, m);
      nb = m;
      if (wave == 1) {
        __hip_atomic_store(&s_decflag, j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);      // (the decode's reads have returned: d.src is formed)
        BSTAMP(5);
        // trie node of every fresh labelling; copies keep the id of the slot they come from
        const int p_id = lane_gather(y_node, d.src);
        int id = p_id;
        if (d.fresh) {
          const int parent = p_id, sym = d.sym;
          id = -1;
          const bool lds_ok = parent <= TS;                           // a child of a global node was created after the overflow
          if (lds_ok) {
            const unsigned entry = ((unsigned)(parent + 1) << 17) | (unsigned)sym;
            // double hashing on the (unique) 32-bit entry: the probe sequence of a key is h, h + step, h + 2 step, ... with an odd step,
            // which visits every slot of the power-of-two table; at 3/4 occupancy the longest of a frame's ~20 probe chains -- what the
            // wave waits for -- is a fraction of what linear probing's clusters gave (ids are slot numbers, nothing else depends on the
            // order).  Multiplicative hashing: the HIGH bits of the products -- the low ones depend on the class and a few parent bits only
            unsigned h = (entry * 0x9E3779B1u) >> tshift;
            const unsigned step = ((entry * 0x85EBCA6Bu) >> tshift) | 1u;
            const bool may_insert = s_gnodes == 0;
            for (int probe = 0; probe < TS; ++probe) {
              unsigned prev = may_insert ? atomicCAS(&trie[h], 0u, entry) : trie[h];
              if (prev == entry) { id = (int)h + 1; break; }
              if (prev == 0u) { if (may_insert) id = (int)h + 1; break; }
              h = (h + step) & tmask;
            }
          }
          if (id < 0) {                                               // global table: {parent : 24 | symbol : 16 | id : 24}
            const unsigned long long key40 = ((unsigned long long)(unsigned)parent << 16) | (unsigned)sym;
            unsigned h = (unsigned)mix64(key40) & htmask;
            int gid = -1;
            for (int probe = 0; probe <= (int)htmask; ++probe) {
              const unsigned long long seen = __hip_atomic_load(&ht[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (seen != HT_EMPTY) {
                if ((seen >> 24) == key40) { id = TS + 1 + (int)(seen & 0xFFFFFFull); break; }
                h = (h + 1) & htmask;
                continue;
              }
              if (gid < 0) gid = atomicAdd(&s_gnodes, 1) - 1;         // s_gnodes = 1 + number of global nodes once overflowed
              const unsigned long long prev = atomicCAS(&ht[h], HT_EMPTY, (key40 << 24) | (unsigned long long)(unsigned)gid);
              if (prev == HT_EMPTY) { id = TS + 1 + gid; if (gid < a.max_nodes) { npar[gid] = parent; nsym[gid] = sym; } break; }
              if ((prev >> 24) == key40) { id = TS + 1 + (int)(prev & 0xFFFFFFull); break; }   // (cannot happen: keys of a frame are distinct)
              h = (h + 1) & htmask;
            }
          }
        }
        {   // LDS trie occupancy: count this frame's fresh lanes; past 3/4 the table is closed for inserts
          const unsigned long long fm = __ballot(d.fresh && id <= TS);
          y_lnodes += __popcll(fm);
          if (lane == 0 && y_lnodes * 4 > TS * 3 && s_gnodes == 0) s_gnodes = 1;
        }
        y_node = d.act ? id : 0;
        nid[(j + 1) & 1][lane] = y_node;
        BSTAMP(6);
      } else if (spec) {
        tots[lane] = sp_half ? sp_x + log(sp_s) : sp_x;
        __hip_atomic_store(&s_totflag, j + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else if (more) {
        // the new slot's (context class, prNonBlank, prTotal) without wave 0: a fresh labelling carries its candidate's score, a copy the
        // stay / merged entry of the slot it comes from (enbv / homev, written by wave 0 before the last barrier; bm_c1 of the old parity)
        const int o_c1 = bm_c1[j & 1][d.src];
        const double o_nb = enbv[d.src], o_t = homev[d.src];
        stay_totals(j + 1, d.act, d.fresh ? d.sym : o_c1, d.fresh ? d.sv : o_nb, d.fresh ? d.sv : o_t);
      }
      fw = fwn;
      lds_barrier();
      BSTAMP(2);
    }
  }
#ifdef CTCN_BEAM_STATS
  if (a.stats && b == 0 && (tid == 0 || tid == 192)) {
    long long *o = a.stats + (tid == 0 ? 0 : 16);
    for (int i = 0; i < 12; ++i) o[i] = zst[i];
    o[12] = zrounds; o[13] = ziters; o[14] = nfl; o[15] = clock64() - zt0;
  }
#endif
  if (wave == 0) f_node[lane] = nid[nfl & 1][lane];
  __syncthreads();
  if (status == 0 && s_fault) status = 4;
  // (f_pT is reused for the scores and f_last for the picks; a node is an LDS trie slot up to TS, an entry of the global table beyond)
  beam_finish<ORDER>(a, b, status, s_gnodes > a.max_nodes, nb, f_len, f_last, f_node, f_pT, f_last, a.lm, [&](int &n) {
    if (n <= TS) { const unsigned e = trie[n - 1]; n = (int)(e >> 17) - 1; return (int)(e & 0x1FFFFu); }
    const int gq = n - TS - 1;
    n = npar[gq];
    return nsym[gq];
  }, f_c0);
}

// the two launch forms of the fast search.  beam_fast_kernel: one workgroup per CU (120 VGPRs, up to 144 KB of dynamic LDS: the 16 K-slot
// trie).  beam_fast_kernel_occ2 (option "beam_occ2"): the same body compiled for eight waves per SIMD (<= 64 VGPRs) and launched with <= 68 KB
// of dynamic LDS, so that TWO utterances share a CU and each one's latency-bound serial chain runs in the other's shadow.
template <int NPT, bool LM_LDS>
__global__ __launch_bounds__(FAST_NTH) void beam_fast_kernel(FastArgs a) { beam_fast_body<NPT, LM_LDS>(a); }
template <int NPT, bool LM_LDS>
__global__ __launch_bounds__(FAST_NTH) __attribute__((amdgpu_waves_per_eu(8, 8))) void beam_fast_kernel_occ2(FastArgs a) { beam_fast_body<NPT, LM_LDS>(a); }
template <int NPT>
__global__ __launch_bounds__(FAST_NTH) void beam_fast_kernel_tri(FastArgs a) { beam_fast_body<NPT, false, 3>(a); }
template <int NPT>
__global__ __launch_bounds__(FAST_NTH) __attribute__((amdgpu_waves_per_eu(8, 8))) void beam_fast_kernel_tri_occ2(FastArgs a) { beam_fast_body<NPT, false, 3>(a); }

// ---- Host side: plan_beam decides a call by arithmetic alone (ctcn_diag_beam_plan shows it to the CPU tests); the entry is check, plan, fill, launch ----
struct BeamOptions { int fast, occ2, generic_threads, cand_global; };
BeamOptions beam_options() {
  return {ctcn_get_option("beam_fast"), ctcn_get_option("beam_occ2"), ctcn_get_option("beam_generic_threads"), ctcn_get_option("beam_cand_global")};
}
enum BeamPath { BP_FAST = 0, BP_FAST_OCC2 = 1, BP_GENERIC = 2 };
// workspace, generic: [hash keys | hash ids | node parents | node symbols | candidate table | node_slot | cand_owner]
//            fast:    [hash table | node parents | node symbols | ln p (T,B,V) double | p_blank (T,B) | log(0) flags (T,B)]
struct BeamWorkspace { size_t ht, ids, npar, nsym, cand, nslot, cown, lgd, pb, zf, total; };
struct BeamPlan {
  BeamPath path;
  int max_nodes, ht_size;                                  // trie nodes per utterance, slots of its global hash table
  int fast_ok, npt, lm_lds, trie_slots; size_t fast_lds;   // the fast kernel's fit and dynamic LDS, whichever path is taken
  int threads, wcap, smax, cand_in_lds, lm_in_lds;         // the generic kernel
  size_t generic_lds; int generic_fits;                    // its dynamic LDS; with its static LDS within lds_max
  BeamWorkspace fast_ws, generic_ws;                       // (ctcn_beam_ws_bytes promises the larger, whatever the options are at decode time)
  size_t lds() const { return path == BP_GENERIC ? generic_lds : fast_lds; }
  const BeamWorkspace &ws() const { return path == BP_GENERIC ? generic_ws : fast_ws; }
};
// (path, threads and the workspaces depend on neither lds_max nor generic_static_lds: the entry plans without them, then asks the device)
// order 3: the (V+1)^3 table stays in global memory on every path (lm_lds = lm_in_lds = 0); the fast kernel's order-3 builds have 768 B
// more static LDS, which the occ2 budget gives back so that two workgroups still share a CU; the generic kernel carries one class more
// per beam slot (GenericLds).
BeamPlan plan_beam(int T, int B, int V, int W, const BeamOptions &o, int lds_max, int generic_static_lds, int order = 2) {
  BeamPlan p = {};
  p.max_nodes = W * T + 2;
  p.ht_size = 1024;
  while (p.ht_size < 2 * p.max_nodes) p.ht_size <<= 1;
  // Fast kernel: of the CU's 160 KB (it also has ~12 KB of static LDS) one workgroup gets 144 KB; occ2: two workgroups per CU, 68 KB each.
  // The LDS trie takes as many slots as fit, at most 16 K (its node ids must fit 14 bits); then the LM if it still fits (occ2 == 2: the LM
  // stays in global memory and the trie gets its share).
  typedef FastLdsT<size_t> Lds;
  p.npt = ceil_div(W * V, FAST_NCT);                       // candidate slots per thread of waves 3..15 (1..4: W * V <= 3 328)
  if (p.npt > 4) p.npt = 0;
  const size_t core = Lds(T, V, W, false, 0).total, lm = Lds::table_bytes(V), budget = o.occ2 ? (order == 3 ? 67 : 68) * 1024 : 144 * 1024;
  const bool want_lm = lm <= 40 * 1024 && o.occ2 != 2 && order == 2;
  p.trie_slots = 16384;
  while (p.trie_slots > 1024 && core + (size_t)p.trie_slots * 4 + (want_lm ? lm : 0) > budget) p.trie_slots >>= 1;
  p.lm_lds = o.occ2 != 2 && order == 2 && core + (size_t)p.trie_slots * 4 + lm <= budget;
  p.fast_lds = Lds(T, V, W, p.lm_lds, p.trie_slots).total;
  p.fast_ok = W <= 60 && p.npt > 0 && V <= 256 && p.max_nodes < (1 << 24) && T < (1 << 22) && p.fast_lds <= budget;
  p.path = (p.fast_ok && o.fast != 0) ? (o.occ2 ? BP_FAST_OCC2 : BP_FAST) : BP_GENERIC;
  // Generic kernel: threads by beam width and candidates per frame, or forced (option beam_generic_threads, for measurements) and then raised
  // to the smallest instantiation >= W -- every beam slot has a thread of its own, so the option never changes a result.  Its dynamic LDS
  // holds what the device's LDS per workgroup leaves room for: the candidate table first (in the workspace otherwise), then the LM table.
  const int need = o.generic_threads == 0 ? ((W > 64 || (long)W * V > 3500) ? 1024 : 256) : std::max(o.generic_threads, W);
  p.threads = need > 512 ? 1024 : need > 256 ? 512 : 256;
  p.wcap = (W + 63) / 64 * 64;
  p.smax = std::max(1024, 2 * p.wcap);
  const size_t cand_bytes = (size_t)W * V * sizeof(double);
  const size_t fixed = (size_t)generic_static_lds + GenericLds(V, W, p.wcap, p.smax, false, false, order).total + 256;
  p.cand_in_lds = fixed + cand_bytes <= (size_t)lds_max && !o.cand_global;
  p.lm_in_lds = order == 2 && fixed + (p.cand_in_lds ? cand_bytes : 0) + GenericLds::table_bytes(V) <= (size_t)lds_max;
  p.generic_lds = GenericLds(V, W, p.wcap, p.smax, p.cand_in_lds, p.lm_in_lds, order).total;
  p.generic_fits = (size_t)generic_static_lds + p.generic_lds <= (size_t)lds_max;
  // workspaces
  const size_t nodes = (size_t)B * p.max_nodes * sizeof(int), slots = (size_t)B * p.ht_size, tb = (size_t)T * B, wv = (size_t)B * W * V;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; };
  BeamWorkspace &f = p.fast_ws, &g = p.generic_ws;
  f.ht = take(slots * 8); f.npar = take(nodes); f.nsym = take(nodes); f.lgd = take(tb * V * sizeof(double)); f.pb = take(tb * sizeof(float));
  f.zf = take(tb); f.total = off;
  off = 0;
  g.ht = take(slots * 8); g.ids = take(slots * sizeof(int)); g.npar = take(nodes); g.nsym = take(nodes); g.cand = take(wv * sizeof(double));
  g.nslot = take(nodes); g.cown = take(wv * sizeof(int)); g.total = off;
  return p;
}
int lds_refused(const BeamPlan &p, int lds_max, int static_lds) {      // the generic kernel is taken and does not fit the device
  if (p.path != BP_GENERIC || p.generic_fits) return CTCN_OK;
  ctcn_set_error("ctcn_beam_decode: %zu B of LDS per workgroup needed, the device gives %d", (size_t)static_lds + p.generic_lds, lds_max);
  return CTCN_EUNSUPPORTED;
}

// instantiations: fast [occ2][lm_lds][npt - 1], generic by thread count; one launch site
#define CTCN_NPT_ROW(K, LM) {K<1, LM>, K<2, LM>, K<3, LM>, K<4, LM>}
void (*const fast_kernels[2][2][4])(FastArgs) = {{CTCN_NPT_ROW(beam_fast_kernel, false), CTCN_NPT_ROW(beam_fast_kernel, true)},
                                                 {CTCN_NPT_ROW(beam_fast_kernel_occ2, false), CTCN_NPT_ROW(beam_fast_kernel_occ2, true)}};
#undef CTCN_NPT_ROW
void (*const fast_kernels_tri[2][4])(FastArgs) = {{beam_fast_kernel_tri<1>, beam_fast_kernel_tri<2>, beam_fast_kernel_tri<3>, beam_fast_kernel_tri<4>},
                                                  {beam_fast_kernel_tri_occ2<1>, beam_fast_kernel_tri_occ2<2>, beam_fast_kernel_tri_occ2<3>,
                                                   beam_fast_kernel_tri_occ2<4>}};       // [occ2][npt - 1]
void (*const generic_kernels[2][3])(BeamArgs) = {{beam_kernel<256, 2>, beam_kernel<512, 2>, beam_kernel<1024, 2>},       // [order - 2][threads / 512]
                                                 {beam_kernel<256, 3>, beam_kernel<512, 3>, beam_kernel<1024, 3>}};
#ifdef CTCN_BEAM_STATS
long long *g_beam_stats_dev = nullptr;
#endif
template <typename Args>
int launch_beam(void (*kern)(Args), int B, int threads, size_t lds, hipStream_t st, Args &a) {
#ifdef CTCN_BEAM_STATS
  if (!g_beam_stats_dev) { CTCN_HIP(hipMalloc(&g_beam_stats_dev, 64 * sizeof(long long))); }
  CTCN_HIP(hipMemsetAsync(g_beam_stats_dev, 0, 64 * sizeof(long long), st));
  a.stats = g_beam_stats_dev;
#endif
  CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(B), dim3(threads), lds, st, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
}  // namespace

extern "C" size_t ctcn_beam_ws_bytes(int T, int B, int V, int W) {
  if (T <= 0 || B <= 0 || V <= 0 || W <= 0) return 0;
  const BeamPlan p = plan_beam(T, B, V, W, beam_options(), 0, 0);
  return std::max(p.generic_ws.total, p.fast_ws.total);
}
// Order of the LM table: 2 = (V+1)^2, 3 = (V+1)^3 of at most TRI_TABLE_MAX bytes (V <= 202; V = 128 is 17 MB).  Refused before any launch.
constexpr size_t TRI_TABLE_MAX = (size_t)64 << 20;
static int order_refused(int lm_order, int V) {
  if (lm_order != 2 && lm_order != 3) { ctcn_set_error("ctcn_beam_decode: LM order %d (2 or 3 are built)", lm_order); return CTCN_EUNSUPPORTED; }
  const size_t bytes = (size_t)(V + 1) * (V + 1) * (V + 1) * sizeof(double);
  if (lm_order == 3 && bytes > TRI_TABLE_MAX) {
    ctcn_set_error("ctcn_beam_decode: an order-3 table of %zu B at V = %d is beyond the cap of %zu B", bytes, V, TRI_TABLE_MAX);
    return CTCN_EUNSUPPORTED;
  }
  return CTCN_OK;
}
extern "C" int ctcn_diag_beam_plan_lm(int T, int B, int V, int W, int lm_order, int lds_max, int generic_static_lds, int *out) {
  CTCN_REQUIRE(out && T > 0 && B > 0 && V > 1 && W >= 1 && W <= BEAM_WMAX && lds_max > 0 && generic_static_lds >= 0, "ctcn_diag_beam_plan: bad args");
  if (const int rc = order_refused(lm_order, V)) return rc;
  const BeamPlan p = plan_beam(T, B, V, W, beam_options(), lds_max, generic_static_lds, lm_order);
  const size_t wf = p.fast_ws.total, wg = p.generic_ws.total;
  const int v[CTCN_BEAM_PLAN_INTS] = {(int)p.path, p.fast_ok, p.npt, p.lm_lds, p.trie_slots, (int)std::min(p.fast_lds, (size_t)INT32_MAX), p.threads, p.wcap,
                                      p.smax, p.cand_in_lds, p.lm_in_lds, (int)std::min(p.generic_lds, (size_t)INT32_MAX), p.generic_fits, p.max_nodes,
                                      p.ht_size, (int)(wf & 0x7fffffff), (int)(wf >> 31), (int)(wg & 0x7fffffff), (int)(wg >> 31)};
  memcpy(out, v, sizeof(v));
  return lds_refused(p, lds_max, generic_static_lds);
}
extern "C" int ctcn_diag_beam_plan(int T, int B, int V, int W, int lds_max, int generic_static_lds, int *out) {
  return ctcn_diag_beam_plan_lm(T, B, V, W, 2, lds_max, generic_static_lds, out);
}

extern "C" int ctcn_beam_decode_lm(const float *x, int input_is_prob, const int32_t *lens, const double *lm, int lm_order, double alpha, int W,
                                   int blank, int nbest, int32_t *out_ids, int32_t *out_len, double *out_score, int32_t *out_count,
                                   int32_t *status, int T, int B, int V, void *ws, size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(x && lens && lm && out_ids && out_len && out_score && status && ws, "ctcn_beam_decode: null pointer");
  CTCN_REQUIRE(T > 0 && B > 0 && V > 1 && blank >= 0 && blank < V, "ctcn_beam_decode: bad dims");
  if (W < 1 || W > BEAM_WMAX) { ctcn_set_error("ctcn_beam_decode: beam width %d outside [1,%d]", W, BEAM_WMAX); return CTCN_EUNSUPPORTED; }
  CTCN_REQUIRE(nbest >= 1 && nbest <= W, "ctcn_beam_decode_nbest: nbest %d outside [1, beam width %d]", nbest, W);
  if (const int rc = order_refused(lm_order, V)) return rc;
  hipStream_t st = (hipStream_t)stream;
  char *base = (char *)ws;
  const BeamOptions o = beam_options();
  BeamPlan p = plan_beam(T, B, V, W, o, 0, 0, lm_order);
  int lds_max = 64 * 1024, static_lds = 0;
  if (p.path == BP_GENERIC) {      // its LDS placement needs two facts of the device: what one workgroup gets, what the instantiation takes statically
    hipFuncAttributes fa;
    CTCN_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(generic_kernels[lm_order - 2][p.threads / 512])));
    int dev_id = 0;
    CTCN_HIP(hipGetDevice(&dev_id));
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev_id) != hipSuccess) lds_max = 64 * 1024;
    static_lds = (int)fa.sharedSizeBytes;
    p = plan_beam(T, B, V, W, o, lds_max, static_lds, lm_order);
  }
  const BeamWorkspace &w = p.ws();
  if (ws_bytes < w.total) { ctcn_set_error("ctcn_beam_decode: workspace too small (%zu < %zu)", ws_bytes, w.total); return CTCN_EWORKSPACE; }
  if (const int rc = lds_refused(p, lds_max, static_lds)) return rc;
  CTCN_HIP(hipMemsetAsync(base + w.ht, 0xFF, (size_t)B * p.ht_size * sizeof(unsigned long long), st));
  auto fill = [&](auto &a) {                     // what both kernels take
    a.lens = lens; a.lm = lm; a.alpha = alpha; a.W = W; a.blank = blank;
    a.out_ids = out_ids; a.out_len = out_len; a.out_score = out_score; a.status = status; a.T = T; a.B = B; a.V = V;
    a.nbest = nbest; a.out_count = out_count;
    a.node_par = (int *)(base + w.npar); a.node_sym = (int *)(base + w.nsym); a.ht_size = p.ht_size; a.max_nodes = p.max_nodes;
  };
  if (p.path != BP_GENERIC) {
    FastArgs a;
    fill(a);
    a.lgd = (const double *)(base + w.lgd); a.pb = (const float *)(base + w.pb); a.zf = (const unsigned char *)(base + w.zf);
    a.ht = (unsigned long long *)(base + w.ht); a.trie_slots = p.trie_slots;
    const size_t rows = (size_t)T * B;
    hipLaunchKernelGGL(beam_prep_kernel, dim3((unsigned)ceil_div_z(rows, 4)), dim3(256), 0, st, x, input_is_prob, (double *)(base + w.lgd),
                       (float *)(base + w.pb), (unsigned char *)(base + w.zf), rows, V, blank);
    CTCN_LAUNCH_CHECK();
    if (lm_order == 3) return launch_beam(fast_kernels_tri[p.path == BP_FAST_OCC2][p.npt - 1], B, FAST_NTH, p.lds(), st, a);
    return launch_beam(fast_kernels[p.path == BP_FAST_OCC2][p.lm_lds][p.npt - 1], B, FAST_NTH, p.lds(), st, a);
  }
  BeamArgs a;
  fill(a);
  a.x = x; a.input_is_prob = input_is_prob; a.ht_keys = (unsigned long long *)(base + w.ht); a.ht_ids = (int *)(base + w.ids);
  a.cand_global = (double *)(base + w.cand); a.node_slot = (int *)(base + w.nslot); a.cand_owner = (int *)(base + w.cown);
  a.wcap = p.wcap; a.smax = p.smax; a.cand_in_lds = p.cand_in_lds; a.lm_in_lds = p.lm_in_lds; a.bitonic = ctcn_get_option("beam_bitonic");
  return launch_beam(generic_kernels[lm_order - 2][p.threads / 512], B, p.threads, p.lds(), st, a);
}

extern "C" int ctcn_beam_decode_nbest(const float *x, int input_is_prob, const int32_t *lens, const double *lm, double alpha, int W,
                                      int blank, int nbest, int32_t *out_ids, int32_t *out_len, double *out_score, int32_t *out_count,
                                      int32_t *status, int T, int B, int V, void *ws, size_t ws_bytes, void *stream) {
  return ctcn_beam_decode_lm(x, input_is_prob, lens, lm, 2, alpha, W, blank, nbest, out_ids, out_len, out_score, out_count, status, T, B, V, ws, ws_bytes, stream);
}

extern "C" int ctcn_beam_decode(const float *x, int input_is_prob, const int32_t *lens, const double *lm, double alpha, int W,
                                int blank, int32_t *out_ids, int32_t *out_len, double *out_score, int32_t *status, int T, int B,
                                int V, void *ws, size_t ws_bytes, void *stream) {
  return ctcn_beam_decode_nbest(x, input_is_prob, lens, lm, alpha, W, blank, 1, out_ids, out_len, out_score, nullptr, status, T, B, V, ws, ws_bytes, stream);
}

#ifdef CTCN_BEAM_STATS
extern "C" int ctcn_beam_stats(long long *host_out) {       // tools/mb_beam.py only
  if (!g_beam_stats_dev) return CTCN_EINVAL;
  CTCN_HIP(hipMemcpy(host_out, g_beam_stats_dev, 64 * sizeof(long long), hipMemcpyDeviceToHost));
  return CTCN_OK;
}
#endif
