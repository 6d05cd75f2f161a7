// cmvn.hip -- mean / variance normalisation: the statistics of all utterances or per group of them (ctcn_cmvn_accumulate,
// ctcn_cmvn_accumulate_groups), their application per group and the sliding window (ctcn_cmvn_apply, ctcn_cmvn_sliding and the host twins
// ctcn_cmvn_norm_host, ctcn_cmvn_sliding_window, ctcn_cmvn_sliding_host; contract in include/ctcn.h, the arithmetic in cmvn_core.h).
//
// cmvn_partial_kernel / cmvn_finish_kernel: float64 column sums of 64-row blocks into the workspace, then one thread per statistic and group
//   adds the group's partials in index order into the caller's block (norm.hip's scheme: no atomics, a function of the input bits).  Without
//   group ids every utterance is in group 0: the global statistics are the grouped ones at G = 1, by the same kernel.
// cmvn_apply_kernel: grid (blocks of 64 rows, utterances), 256 threads laid out as (256 / CW rows, CW columns), CW in {64, 128, 256} chosen
//   from F so that few lanes idle.  A thread forms mean and scale of its column from the group's statistics in double (a division, a square
//   root and a reciprocal: ~150 instructions, against 64 / (256 / CW) elements of 3 each), then walks the block's rows of that column:
//   consecutive lanes on consecutive floats, every element read and written by the same thread (so out may be feats), rows at or beyond
//   the utterance's length zero-filled without a read.
// cmvn_sliding_kernel: one wave per (64 columns, utterance); lane = column, so a row load is one coalesced 256-byte request.  The chain in
//   time is S -= leaving, S += entering (and the same for Q): two dependent float64 additions per frame.  Everything else hangs off it: the
//   division S / w, the variance and its square root depend on S_t but nothing depends on them, so they overlap with the next frames' sums.
//   Row loads are kept off the chain by staging: time runs in runs of CMVN_RUN frames; for each frame of a run the wave holds three
//   registers -- the frame itself, the frame that leaves the window and the frame that enters it (the window rule is wave-uniform scalar
//   arithmetic on t and n alone, so all 3 x CMVN_RUN addresses of a run are known before any value is) -- in two sets that swap roles:
//   the loads of run k + 1 are issued before the sums of run k are touched, and a trip of the loop is ONE basic block (variance and
//   centring are template parameters, a bound that does not move contributes +0.0 instead of a branch), so the compiler counts its waits
//   per load and leaves the run's 16 stores in flight.  (A first build with a branch per frame waited for vmcnt(0) -- the previous frame's
//   store included -- in front of every frame: 400 ns per frame.)  A frame behind the utterance is never loaded.  The frames behind the
//   last whole run (fewer than CMVN_RUN) are walked one by one.  The first window is summed in ascending order, eight loads in flight.
#include "cmvn_core.h"
#include "common.h"

namespace {

constexpr int CMVN_ROWS = 64;                      // rows of a block of cmvn_partial_kernel
constexpr int CMVN_APPLY_ROWS = 64;
constexpr int CMVN_RUN = 16;                       // frames staged at a time by cmvn_sliding_kernel (ctcn_cmvn_sliding_run)
constexpr int CMVN_MAX_FRAMES = 1 << 30;

// Partial sums of rows [c * 64, c * 64 + 64) below frames[b] of utterance b: ws[(b * chunks + c)][2][F] doubles (zeros for an empty block).
__global__ __launch_bounds__(256) void cmvn_partial_kernel(const float *__restrict__ feats, const int32_t *__restrict__ frames, double *__restrict__ ws,
                                                           int Tmax, int F) {
  const int b = blockIdx.y, c = blockIdx.x, chunks = gridDim.x;
  const int Tb = min(max(frames[b], 0), Tmax);
  const int t0 = c * CMVN_ROWS, t1 = min(t0 + CMVN_ROWS, Tb);
  double *o = ws + ((size_t)b * chunks + c) * 2 * F;
  const float *x = feats + (size_t)b * Tmax * F;
  for (int f = threadIdx.x; f < F; f += 256) {
    double s = 0.0, q = 0.0;
    for (int t = t0; t < t1; ++t) {
      const double v = (double)x[(size_t)t * F + f];
      s += v;
      q += v * v;
    }
    o[f] = s;
    o[F + f] = q;
  }
}

// Grid (statistics / 256, groups).  Thread i < 2F of group g adds its column of the partials of the utterances of group g (group[b] == g;
// GROUPED == false: no ids, every utterance is in group 0), in ascending (utterance, block) order, into stats[g]; thread 2F their frame
// counts in ascending utterance order.  (A template parameter, not a test of `group`: the walk over the utterances is one wave's dependent chain.)
template <bool GROUPED>
__global__ __launch_bounds__(256) void cmvn_finish_kernel(const double *__restrict__ ws, const int32_t *__restrict__ frames,
                                                          const int32_t *__restrict__ group, double *__restrict__ stats, int B, int Tmax, int F,
                                                          int chunks) {
  const int i = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  double *st = stats + (size_t)g * 2 * (F + 1);
  if (i < 2 * F) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      if ((GROUPED ? group[b] : 0) != g) continue;
      const double *p = ws + (size_t)b * chunks * 2 * F + i;
#pragma unroll 8
      for (int c = 0; c < chunks; ++c) s += p[(size_t)c * 2 * F];   // the loads do not wait for the sum: eight in flight, added in order
    }
    st[i < F ? i : i + 1] += s;                                       // row 1 starts at F + 1
  } else if (i == 2 * F) {
    double cnt = 0.0;
    for (int b = 0; b < B; ++b)
      if ((GROUPED ? group[b] : 0) == g) cnt += (double)min(max(frames[b], 0), Tmax);
    st[F] += cnt;
  }
}

__global__ __launch_bounds__(256) void cmvn_apply_kernel(const float *feats, const int32_t *__restrict__ frames, const int32_t *__restrict__ group,
                                                         const double *__restrict__ stats, float *out, int Tmax, int F, int G, int norm_vars,
                                                         int cw_shift) {
  const int b = blockIdx.y;
  const int n = min(max(frames[b], 0), Tmax);
  const int t0 = blockIdx.x * CMVN_APPLY_ROWS, t1 = min(t0 + CMVN_APPLY_ROWS, Tmax);
  const int cw = 1 << cw_shift, c = threadIdx.x & (cw - 1), r = threadIdx.x >> cw_shift, rstep = 256 >> cw_shift;
  const int g = group ? group[b] : 0;
  const double *st = (g >= 0 && g < G) ? stats + (size_t)g * 2 * (F + 1) : nullptr;
  const double cnt = (st && t0 < n) ? st[F] : 0.0;                    // a block of padding needs no statistics
  const size_t base = (size_t)b * Tmax * F;
  for (int f = c; f < F; f += cw) {
    float mean = 0.f, scale = 1.f;
    if (cnt > 0.0) cmvn_norm(st[f], st[F + 1 + f], cnt, norm_vars, &mean, &scale);
    for (int t = t0 + r; t < t1; t += rstep) {
      const size_t i = base + (size_t)t * F + f;
      out[i] = t < n ? (cnt > 0.0 ? cmvn_apply_one(feats[i], mean, scale) : feats[i]) : 0.f;
    }
  }
}

struct SlideRows {
  float cur[CMVN_RUN], lead[CMVN_RUN], trail[CMVN_RUN];
  int w[CMVN_RUN];                                 // wave-uniform: the window's size per frame, and which bounds moved
  unsigned drop, gain;
};

// The loads of the run of frames [t0, t0 + CMVN_RUN), all of them below n: the frame, the frame the window drops and the frame it gains.
// No branch: a bound that does not move loads the frame itself (a row that is there); slide_run turns that value into +0.0f where it uses
// it, so that nothing here waits for a load.  The window rule runs once per frame, here, on the scalar unit; slide_run reads its results.
template <bool CENTER>
__device__ __forceinline__ void slide_load(SlideRows &r, const float *__restrict__ x, int F, int t0, int n, int window, int min_window) {
  int s0, e0;
  cmvn_window(max(t0 - 1, 0), n, window, min_window, CENTER, &s0, &e0);
  r.drop = r.gain = 0u;
#pragma unroll
  for (int i = 0; i < CMVN_RUN; ++i) {
    const int t = t0 + i;
    int s1, e1;
    cmvn_window(t, n, window, min_window, CENTER, &s1, &e1);         // t = 0: the same window twice, nothing moves
    r.cur[i] = x[(size_t)t * F];
    r.trail[i] = x[(size_t)(s1 > s0 ? s0 : t) * F];                   // s0 < s1 < e1 <= n
    r.lead[i] = x[(size_t)(e1 > e0 ? e0 : t) * F];                    // e0 < e1 <= n
    r.drop |= (unsigned)(s1 > s0) << i;
    r.gain |= (unsigned)(e1 > e0) << i;
    r.w[i] = e1 - s1;
    s0 = s1; e0 = e1;
  }
}

// The frames of one staged run.  S and Q never hold -0.0 -- they start from +0.0, and in round-to-nearest a sum is -0.0 only when both
// operands are -0.0 -- so subtracting or adding the +0.0 of a bound that did not move leaves their bits alone: the contract's conditional
// update without a branch or a select on the chain.
template <bool NV>
__device__ __forceinline__ void slide_run(const SlideRows &r, float *__restrict__ o, int F, int t0, double &S, double &Q) {
#pragma unroll
  for (int i = 0; i < CMVN_RUN; ++i) {
    cmvn_slide_sub(&S, &Q, (r.drop >> i) & 1u ? r.trail[i] : 0.f);
    cmvn_slide_add(&S, &Q, (r.gain >> i) & 1u ? r.lead[i] : 0.f);
    o[(size_t)(t0 + i) * F] = cmvn_slide_out(r.cur[i], S, Q, r.w[i], NV);
  }
}

template <bool NV, bool CENTER>
__global__ __launch_bounds__(64) void cmvn_sliding_kernel(const float *__restrict__ feats, const int32_t *__restrict__ frames, float *__restrict__ out,
                                                          int Tmax, int F, int window, int min_window) {
  const int b = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;                                                 // no barrier and no cross-lane operation below
  const int n = min(max(frames[b], 0), Tmax);
  const float *x = feats + (size_t)b * Tmax * F + f;
  float *o = out + (size_t)b * Tmax * F + f;
  if (n > 0) {
    const int full = n / CMVN_RUN;                                    // whole runs; the frames behind them are walked one by one
    SlideRows A, B;
    if (full > 0) slide_load<CENTER>(A, x, F, 0, n, window, min_window);
    int s, e;
    cmvn_window(0, n, window, min_window, CENTER, &s, &e);
    double S = 0.0, Q = 0.0;
#pragma unroll 8
    for (int u = s; u < e; ++u) cmvn_slide_add(&S, &Q, x[(size_t)u * F]);
    // Two runs per trip, the register sets swapping roles, so that nothing is copied and the loads of a run are issued a whole run ahead of
    // their use.  A prefetch past the last whole run loads the last whole run again (rows that are there) instead of branching.
    int k = 0;
    for (; k + 1 < full; k += 2) {
      slide_load<CENTER>(B, x, F, (k + 1) * CMVN_RUN, n, window, min_window);
      slide_run<NV>(A, o, F, k * CMVN_RUN, S, Q);
      slide_load<CENTER>(A, x, F, min(k + 2, full - 1) * CMVN_RUN, n, window, min_window);
      slide_run<NV>(B, o, F, (k + 1) * CMVN_RUN, S, Q);
    }
    if (k < full) slide_run<NV>(A, o, F, k * CMVN_RUN, S, Q);
    for (int t = full * CMVN_RUN; t < n; ++t) {                       // fewer than CMVN_RUN frames: loaded where they are used
      if (t > 0) {
        int s0, e0;
        cmvn_window(t - 1, n, window, min_window, CENTER, &s0, &e0);
        cmvn_window(t, n, window, min_window, CENTER, &s, &e);
        if (s > s0) cmvn_slide_sub(&S, &Q, x[(size_t)s0 * F]);
        if (e > e0) cmvn_slide_add(&S, &Q, x[(size_t)e0 * F]);
      }
      o[(size_t)t * F] = cmvn_slide_out(x[(size_t)t * F], S, Q, e - s, NV);
    }
  }
  for (int t = n; t < Tmax; ++t) o[(size_t)t * F] = 0.f;
}

int sliding_opts_ok(const ctcn_sliding_cmn_opts *opts, const char **why) {
  if (!opts) { *why = "null options"; return CTCN_EINVAL; }
  if (opts->cmn_window < 1) { *why = "cmn_window below 1"; return CTCN_EINVAL; }
  if (opts->min_cmn_window < 1 || opts->min_cmn_window > opts->cmn_window) { *why = "min_cmn_window outside [1, cmn_window]"; return CTCN_EINVAL; }
  return CTCN_OK;
}

size_t accumulate_ws_bytes(int B, int Tmax, int F) { return (size_t)B * ceil_div(Tmax, CMVN_ROWS) * 2 * F * sizeof(double); }

// Both accumulate entry points behind their own argument checks: alignment and workspace under the caller's name, the partial sums, the
// finish per group.  group == nullptr (ctcn_cmvn_accumulate): no ids, one group (G = 1) holding every utterance.
int cmvn_accumulate(const char *who, const float *feats, const int32_t *frames, const int32_t *group, double *stats, int B, int Tmax, int F, int G,
                    void *ws, size_t ws_bytes, void *stream) {
  const size_t need = accumulate_ws_bytes(B, Tmax, F);
  CTCN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)stats & 7) == 0, "%s: workspace of ctcn_cmvn_accumulate_ws_bytes needed, 8-byte aligned", who);
  if (ws_bytes < need) { ctcn_set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need); return CTCN_EWORKSPACE; }
  const int chunks = ceil_div(Tmax, CMVN_ROWS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cmvn_partial_kernel, dim3(chunks, B), dim3(256), 0, st, feats, frames, static_cast<double *>(ws), Tmax, F);
  CTCN_LAUNCH_CHECK();
  hipLaunchKernelGGL(group ? cmvn_finish_kernel<true> : cmvn_finish_kernel<false>, dim3(ceil_div(2 * F + 1, 256), G), dim3(256), 0, st,
                     static_cast<const double *>(ws), frames, group, stats, B, Tmax, F, chunks);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

}  // namespace

extern "C" size_t ctcn_cmvn_accumulate_ws_bytes(int B, int Tmax, int F) { return B <= 0 || Tmax <= 0 || F <= 0 ? 0 : accumulate_ws_bytes(B, Tmax, F); }

extern "C" int ctcn_cmvn_accumulate(const float *feats, const int32_t *frames, double *stats, int B, int Tmax, int F, void *ws, size_t ws_bytes,
                                    void *stream) {
  CTCN_REQUIRE(feats && frames && stats && B > 0 && Tmax > 0 && F > 0 && B <= 65535, "ctcn_cmvn_accumulate: bad args");
  return cmvn_accumulate("ctcn_cmvn_accumulate", feats, frames, nullptr, stats, B, Tmax, F, 1, ws, ws_bytes, stream);
}

extern "C" int ctcn_cmvn_accumulate_groups(const float *feats, const int32_t *frames, const int32_t *group, double *stats, int B, int Tmax, int F,
                                           int G, void *ws, size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(feats && frames && group && stats && B > 0 && Tmax > 0 && F > 0 && B <= 65535 && G > 0 && G <= 65535,
               "ctcn_cmvn_accumulate_groups: bad args (B %d and G %d at most 65 535)", B, G);
  return cmvn_accumulate("ctcn_cmvn_accumulate_groups", feats, frames, group, stats, B, Tmax, F, G, ws, ws_bytes, stream);
}

extern "C" int ctcn_cmvn_apply(const float *feats, const int32_t *frames, const int32_t *group, const double *stats, float *out, int B, int Tmax,
                               int F, int G, int norm_vars, void *stream) {
  CTCN_REQUIRE(feats && frames && stats && out && B > 0 && B <= 65535 && Tmax > 0 && Tmax <= CMVN_MAX_FRAMES && F > 0 && G > 0,
               "ctcn_cmvn_apply: bad args (B %d at most 65 535, Tmax %d at most 2^30, F %d, G %d)", B, Tmax, F, G);
  CTCN_REQUIRE(((uintptr_t)stats & 7) == 0, "ctcn_cmvn_apply: stats must be 8-byte aligned");
  const size_t bytes = (size_t)B * Tmax * F * sizeof(float);
  const uintptr_t a = (uintptr_t)feats, o = (uintptr_t)out;
  CTCN_REQUIRE(a == o || a + bytes <= o || o + bytes <= a, "ctcn_cmvn_apply: out may be feats itself, not a shifted overlap of it");
  const int cw_shift = F <= 64 ? 6 : F <= 128 ? 7 : 8;
  hipLaunchKernelGGL(cmvn_apply_kernel, dim3(ceil_div(Tmax, CMVN_APPLY_ROWS), B), dim3(256), 0, (hipStream_t)stream, feats, frames, group, stats, out,
                     Tmax, F, G, norm_vars != 0, cw_shift);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_cmvn_sliding_run(const ctcn_sliding_cmn_opts *opts) {
  const char *why;
  const int rc = sliding_opts_ok(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_cmvn_sliding_run: %s", why); return rc; }
  return CMVN_RUN;
}

extern "C" int ctcn_cmvn_sliding_window(int t, int n, const ctcn_sliding_cmn_opts *opts, int32_t *start, int32_t *end) {
  const char *why;
  const int rc = sliding_opts_ok(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_cmvn_sliding_window: %s", why); return rc; }
  CTCN_REQUIRE(start && end && n >= 1 && n <= CMVN_MAX_FRAMES && t >= 0 && t < n, "ctcn_cmvn_sliding_window: bad args (frame %d of %d)", t, n);
  int s, e;
  cmvn_window(t, n, opts->cmn_window, opts->min_cmn_window, opts->center != 0, &s, &e);
  *start = s;
  *end = e;
  return CTCN_OK;
}

extern "C" int ctcn_cmvn_sliding(const float *feats, const int32_t *frames, float *out, int B, int Tmax, int F, const ctcn_sliding_cmn_opts *opts,
                                 void *stream) {
  const char *why;
  const int rc = sliding_opts_ok(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_cmvn_sliding: %s", why); return rc; }
  CTCN_REQUIRE(feats && frames && out && B > 0 && B <= 65535 && Tmax > 0 && Tmax <= CMVN_MAX_FRAMES && F > 0 && F <= 64 * 65535,
               "ctcn_cmvn_sliding: bad args (B %d at most 65 535, Tmax %d at most 2^30, F %d)", B, Tmax, F);
  const size_t bytes = (size_t)B * Tmax * F * sizeof(float);
  const uintptr_t a = (uintptr_t)feats, o = (uintptr_t)out;
  CTCN_REQUIRE(a + bytes <= o || o + bytes <= a, "ctcn_cmvn_sliding: out must not overlap feats (the window reads frames behind the one it writes)");
  const dim3 grid(ceil_div(F, 64), B);
  const bool nv = opts->normalize_variance != 0, center = opts->center != 0;
  auto kernel = nv ? (center ? cmvn_sliding_kernel<true, true> : cmvn_sliding_kernel<true, false>)
                   : (center ? cmvn_sliding_kernel<false, true> : cmvn_sliding_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(64), 0, (hipStream_t)stream, feats, frames, out, Tmax, F, opts->cmn_window, opts->min_cmn_window);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_cmvn_sliding_host(const float *feats, int num_frames, int F, const ctcn_sliding_cmn_opts *opts, float *out) {
  const char *why;
  const int rc = sliding_opts_ok(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_cmvn_sliding_host: %s", why); return rc; }
  const int n = num_frames;
  CTCN_REQUIRE(n >= 0 && n <= CMVN_MAX_FRAMES && F > 0 && ((feats && out) || n == 0), "ctcn_cmvn_sliding_host: bad args (frames %d, F %d)", n, F);
  const size_t bytes = (size_t)n * F * sizeof(float);
  const uintptr_t a = (uintptr_t)feats, o = (uintptr_t)out;
  CTCN_REQUIRE(n == 0 || a + bytes <= o || o + bytes <= a, "ctcn_cmvn_sliding_host: out must not overlap feats");
  const int window = opts->cmn_window, min_window = opts->min_cmn_window, center = opts->center != 0, norm_vars = opts->normalize_variance != 0;
  for (int f = 0; f < F && n > 0; ++f) {
    const float *x = feats + f;
    int s, e;
    cmvn_window(0, n, window, min_window, center, &s, &e);
    double S = 0.0, Q = 0.0;
    for (int u = s; u < e; ++u) cmvn_slide_add(&S, &Q, x[(size_t)u * F]);
    for (int t = 0; t < n; ++t) {
      if (t > 0) {
        int s1, e1;
        cmvn_window(t, n, window, min_window, center, &s1, &e1);
        if (s1 > s) cmvn_slide_sub(&S, &Q, x[(size_t)s * F]);
        if (e1 > e) cmvn_slide_add(&S, &Q, x[(size_t)e * F]);
        s = s1; e = e1;
      }
      out[(size_t)t * F + f] = cmvn_slide_out(x[(size_t)t * F], S, Q, e - s, norm_vars);
    }
  }
  return CTCN_OK;
}

extern "C" int ctcn_cmvn_norm_host(const double *stats, int F, int norm_vars, float *mean, float *scale) {
  CTCN_REQUIRE(stats && mean && scale && F > 0, "ctcn_cmvn_norm_host: bad args (F %d)", F);
  const double n = stats[F];
  CTCN_REQUIRE(n > 0.0, "ctcn_cmvn_norm_host: no frames accumulated (count %g)", n);
  for (int f = 0; f < F; ++f) cmvn_norm(stats[f], stats[F + 1 + f], n, norm_vars != 0, &mean[f], &scale[f]);
  return CTCN_OK;
}
