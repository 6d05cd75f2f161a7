// specaug.hip -- SpecAugment on a padded batch of base features, the stage in front of context.hip: time warp, frequency masks and time
// masks, redrawn per utterance from Philox (ctcn_spec_augment; ctcn_spec_augment_plan, the intervals of one utterance on the host;
// ctcn_spec_augment_host, the same computation for one utterance on the host; the computation step by step in include/ctcn.h).
//
// spec_augment_kernel: grid (tiles of SPECAUG_TILE_ROWS rows, utterances), four waves per workgroup.
//   1. A tile at or beyond the utterance's length is zeros: written and done, nothing drawn.
//   2. Lanes 0 .. 40 of the first wave each make ONE Philox call -- lane d is draw d: 0 the warp, 1 .. 8 the frequency masks, 9 .. 40 the time
//      masks -- and park (start, length) in LDS; a draw that is switched off parks (0, 0).
//   3. One lane per row of the tile classifies it once: zeros (t >= T), fill (inside a time mask: its source is never read), copy (the
//      warp lands on a frame) or interpolate, with the two source rows and the float64 weight.  The int64 divisions happen here, not per element.
//   4. Every output element of the tile, lane after lane on consecutive floats: fill inside a frequency mask, else the row's value.
// The host entry points run the same specaug_interval / specaug_source / specaug_lerp: one definition of the arithmetic.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

constexpr int SPECAUG_TILE_ROWS = 32;
constexpr int SPECAUG_MAX_FREQ_MASKS = 8;
constexpr int SPECAUG_MAX_TIME_MASKS = 32;
constexpr int SPECAUG_TIME_DRAW0 = 1 + SPECAUG_MAX_FREQ_MASKS;                        // 9: the first time mask's draw
constexpr int SPECAUG_DRAWS = SPECAUG_TIME_DRAW0 + SPECAUG_MAX_TIME_MASKS;            // 41: one lane each
constexpr int SPECAUG_MAX_DIM = 1 << 16;           // F
constexpr int SPECAUG_MAX_FRAMES = 1 << 30;
enum { SPECAUG_ZERO = 0, SPECAUG_FILL = 1, SPECAUG_COPY = 2, SPECAUG_LERP = 3 };

static int specaug_check(const ctcn_specaug_opts *o, int F, const char **why) {
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (o->warp_window < 0 || o->num_freq_masks < 0 || o->freq_width < 0 || o->num_time_masks < 0 || o->time_width < 0) {
    *why = "warp_window, the mask counts and the mask widths must not be negative";
    return CTCN_EINVAL;
  }
  if (!(o->time_ratio >= 0.f && o->time_ratio <= 1.f)) { *why = "time_ratio outside [0, 1]"; return CTCN_EINVAL; }
  if (!std::isfinite(o->fill)) { *why = "fill is not finite"; return CTCN_EINVAL; }
  if (F < 1) { *why = "F must be positive"; return CTCN_EINVAL; }
  if (o->num_freq_masks > SPECAUG_MAX_FREQ_MASKS) { *why = "more than 8 frequency masks"; return CTCN_EUNSUPPORTED; }
  if (o->num_time_masks > SPECAUG_MAX_TIME_MASKS) { *why = "more than 32 time masks"; return CTCN_EUNSUPPORTED; }
  if (F > SPECAUG_MAX_DIM) { *why = "more than 65 536 columns"; return CTCN_EUNSUPPORTED; }
  return CTCN_OK;
}

__host__ __device__ __forceinline__ int specaug_min(int a, int b) { return a < b ? a : b; }

// rnd(word, n) of the contract: an integer in [0, n), n >= 1, from the word's upper 24 bits.
__host__ __device__ __forceinline__ int specaug_rnd(uint32_t word, int n) { return (int)(((uint64_t)(word >> 8) * (uint64_t)(uint32_t)n) >> 24); }

// Draw d of utterance u (T frames, F columns): (start, len) of a mask, (c, w) of the warp; (0, 0) where the options switch that draw off.
__host__ __device__ inline void specaug_interval(const ctcn_specaug_opts &o, uint64_t seed, uint64_t u, int d, int T, int F, int *start, int *len) {
  *start = 0;
  *len = 0;
  const bool warp = d == 0 && o.warp_window > 0 && (long long)T > 2LL * o.warp_window;
  const bool freq = d >= 1 && d <= o.num_freq_masks;
  const bool time = d >= SPECAUG_TIME_DRAW0 && d < SPECAUG_TIME_DRAW0 + o.num_time_masks;
  if (!warp && !freq && !time) return;
  uint32_t r[4];
  philox4(seed, (u << 8) | (uint64_t)d, r);
  if (warp) {
    const int W = o.warp_window;
    const int c = W + specaug_rnd(r[0], T - 2 * W);
    *start = c;
    *len = c + specaug_rnd(r[1], 2 * W - 1) - (W - 1);
  } else if (freq) {
    const int n = specaug_rnd(r[0], specaug_min(o.freq_width, F) + 1);
    *len = n;
    *start = specaug_rnd(r[1], F - n + 1);
  } else {
    const int cap = specaug_min(specaug_min(o.time_width, T), (int)floor((double)o.time_ratio * (double)T));
    const int n = specaug_rnd(r[0], cap + 1);
    *len = n;
    *start = specaug_rnd(r[1], T - n + 1);
  }
}

// Source of output row t < T under the warp (c, w); w = 0: no warp.  Returns true where the row interpolates rows i0 and i1 with weight a.
__host__ __device__ inline bool specaug_source(int t, int T, int c, int w, int *i0, int *i1, double *a) {
  *i0 = *i1 = t;
  *a = 0.0;
  if (w <= 0) return false;
  long long num, den, base;
  if (t < w) { num = (long long)t * c; den = w; base = 0; }
  else { num = (long long)(t - w) * (T - c); den = T - w; base = c; }
  const long long q = num / den, rem = num - q * den;
  *i0 = (int)(base + q);
  *i1 = specaug_min(*i0 + 1, T - 1);
  if (rem == 0) return false;
  *a = (double)rem / (double)den;
  return true;
}

__host__ __device__ __forceinline__ float specaug_lerp(double a, float x0, float x1) {
#pragma clang fp contract(off)                                        // two products and a sum, each rounded on its own: numpy's bits
  const double p0 = (1.0 - a) * (double)x0;
  const double p1 = a * (double)x1;
  return (float)(p0 + p1);
}

struct SpecArgs {
  const float *feats;
  const int32_t *frames;
  float *out;
  ctcn_specaug_opts o;
  uint64_t seed, utt_offset;
  int Tmax, F;
};

__global__ __launch_bounds__(256) void spec_augment_kernel(SpecArgs a) {
  __shared__ int iv[SPECAUG_DRAWS][2];
  __shared__ int row_kind[SPECAUG_TILE_ROWS], row_i0[SPECAUG_TILE_ROWS], row_i1[SPECAUG_TILE_ROWS];
  __shared__ double row_a[SPECAUG_TILE_ROWS];
  const int b = blockIdx.y, tid = threadIdx.x, F = a.F;
  const int T = min(max(a.frames[b], 0), a.Tmax);
  const int r0 = blockIdx.x * SPECAUG_TILE_ROWS;
  const int nrows = min(SPECAUG_TILE_ROWS, a.Tmax - r0);                // rows of this tile inside the batch
  if (nrows <= 0) return;
  const int n = nrows * F;
  float *out = a.out + ((size_t)b * a.Tmax + r0) * F;
  if (r0 >= T) {                                                       // (the whole workgroup)
    for (int i = tid; i < n; i += 256) out[i] = 0.f;
    return;
  }
  if (tid < SPECAUG_DRAWS) specaug_interval(a.o, a.seed, a.utt_offset + (uint64_t)b, tid, T, F, &iv[tid][0], &iv[tid][1]);
  __syncthreads();
  const int nf = a.o.num_freq_masks, nt = a.o.num_time_masks;
  if (tid < nrows) {
    const int t = r0 + tid;
    int kind = SPECAUG_ZERO, i0 = 0, i1 = 0;
    double w = 0.0;
    if (t < T) {
      bool masked = false;
      for (int k = 0; k < nt; ++k) masked |= (unsigned)(t - iv[SPECAUG_TIME_DRAW0 + k][0]) < (unsigned)iv[SPECAUG_TIME_DRAW0 + k][1];
      if (masked) kind = SPECAUG_FILL;
      else kind = specaug_source(t, T, iv[0][0], iv[0][1], &i0, &i1, &w) ? SPECAUG_LERP : SPECAUG_COPY;
    }
    row_kind[tid] = kind; row_i0[tid] = i0; row_i1[tid] = i1; row_a[tid] = w;
  }
  __syncthreads();
  const float *src = a.feats + (size_t)b * a.Tmax * F;
  const float fill = a.o.fill;
  for (int i = tid; i < n; i += 256) {
    const int r = i / F, f = i - r * F;
    const int kind = row_kind[r];
    float v = 0.f;
    if (kind != SPECAUG_ZERO) {
      bool masked = kind == SPECAUG_FILL;
      for (int k = 1; k <= nf; ++k) masked |= (unsigned)(f - iv[k][0]) < (unsigned)iv[k][1];
      if (masked) v = fill;
      else if (kind == SPECAUG_COPY) v = src[(size_t)row_i0[r] * F + f];
      else v = specaug_lerp(row_a[r], src[(size_t)row_i0[r] * F + f], src[(size_t)row_i1[r] * F + f]);
    }
    out[i] = v;
  }
}

struct SpecPlan {
  int c, w;
  int f0[SPECAUG_MAX_FREQ_MASKS], flen[SPECAUG_MAX_FREQ_MASKS];
  int t0[SPECAUG_MAX_TIME_MASKS], tlen[SPECAUG_MAX_TIME_MASKS];
};

static void specaug_plan(const ctcn_specaug_opts &o, uint64_t seed, uint64_t u, int T, int F, SpecPlan *p) {
  specaug_interval(o, seed, u, 0, T, F, &p->c, &p->w);
  for (int k = 0; k < o.num_freq_masks; ++k) specaug_interval(o, seed, u, 1 + k, T, F, &p->f0[k], &p->flen[k]);
  for (int k = 0; k < o.num_time_masks; ++k) specaug_interval(o, seed, u, SPECAUG_TIME_DRAW0 + k, T, F, &p->t0[k], &p->tlen[k]);
}

}  // namespace

extern "C" int ctcn_spec_augment(const float *feats, const int32_t *frames, const ctcn_specaug_opts *opts, uint64_t seed, uint64_t utt_offset,
                                 float *out, int B, int Tmax, int F, void *stream) {
  const char *why;
  const int rc = specaug_check(opts, F, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_spec_augment: %s", why); return rc; }
  CTCN_REQUIRE(frames && B > 0 && B <= 65535 && Tmax >= 0 && Tmax <= SPECAUG_MAX_FRAMES && ((feats && out) || Tmax == 0),
               "ctcn_spec_augment: bad args (B %d at most 65 535, Tmax %d at most 2^30)", B, Tmax);
  CTCN_REQUIRE(feats != out || Tmax == 0, "ctcn_spec_augment: out must not alias feats (the warp gathers)");
  if (Tmax == 0) return CTCN_OK;
  SpecArgs a;
  a.feats = feats; a.frames = frames; a.out = out; a.o = *opts; a.seed = seed; a.utt_offset = utt_offset; a.Tmax = Tmax; a.F = F;
  hipLaunchKernelGGL(spec_augment_kernel, dim3(ceil_div(Tmax, SPECAUG_TILE_ROWS), B), dim3(256), 0, (hipStream_t)stream, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_spec_augment_plan(const ctcn_specaug_opts *opts, uint64_t seed, uint64_t utt_index, int T, int F, int32_t *warp, int32_t *freq,
                                      int32_t *time) {
  const char *why;
  const int rc = specaug_check(opts, F, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_spec_augment_plan: %s", why); return rc; }
  CTCN_REQUIRE(T >= 0 && T <= SPECAUG_MAX_FRAMES && warp && (freq || opts->num_freq_masks == 0) && (time || opts->num_time_masks == 0),
               "ctcn_spec_augment_plan: bad args (T %d at most 2^30)", T);
  SpecPlan p;
  specaug_plan(*opts, seed, utt_index, T, F, &p);
  warp[0] = p.c; warp[1] = p.w;
  for (int k = 0; k < opts->num_freq_masks; ++k) { freq[2 * k] = p.f0[k]; freq[2 * k + 1] = p.flen[k]; }
  for (int k = 0; k < opts->num_time_masks; ++k) { time[2 * k] = p.t0[k]; time[2 * k + 1] = p.tlen[k]; }
  return CTCN_OK;
}

extern "C" int ctcn_spec_augment_host(const float *feats, int T, int F, const ctcn_specaug_opts *opts, uint64_t seed, uint64_t utt_index,
                                      float *out) {
  const char *why;
  const int rc = specaug_check(opts, F, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_spec_augment_host: %s", why); return rc; }
  CTCN_REQUIRE(T >= 0 && T <= SPECAUG_MAX_FRAMES && ((feats && out) || T == 0), "ctcn_spec_augment_host: bad args (T %d at most 2^30)", T);
  CTCN_REQUIRE(feats != out || T == 0, "ctcn_spec_augment_host: out must not alias feats (the warp gathers)");
  SpecPlan p;
  specaug_plan(*opts, seed, utt_index, T, F, &p);
  for (int t = 0; t < T; ++t) {
    float *orow = out + (size_t)t * F;
    bool masked = false;
    for (int k = 0; k < opts->num_time_masks; ++k) masked |= t >= p.t0[k] && t < p.t0[k] + p.tlen[k];
    if (masked) {
      for (int f = 0; f < F; ++f) orow[f] = opts->fill;
      continue;
    }
    int i0, i1;
    double a;
    const bool lerp = specaug_source(t, T, p.c, p.w, &i0, &i1, &a);
    const float *x0 = feats + (size_t)i0 * F, *x1 = feats + (size_t)i1 * F;
    for (int f = 0; f < F; ++f) orow[f] = lerp ? specaug_lerp(a, x0[f], x1[f]) : x0[f];
    for (int k = 0; k < opts->num_freq_masks; ++k)
      for (int f = p.f0[k]; f < p.f0[k] + p.flen[k]; ++f) orow[f] = opts->fill;
  }
  return CTCN_OK;
}
