// context.hip -- the stage between the feature kernels and the model: Kaldi's add-deltas, frame splicing, frame skipping and the zero rows
// that pad an utterance to a multiple of n_downsample, for a whole padded batch in one launch (ctcn_context_frames, ctcn_delta_scales,
// ctcn_frame_context_tile, ctcn_frame_context; ctcn_frame_context_host, the same computation for one utterance on the host; the computation
// step by step in include/ctcn.h).
//
// frame_context_kernel: grid (tiles of output rows, utterances), four waves per workgroup.
//   A tile is `rows` output rows r0 .. r0 + rows.  Kept row r is frame t = r skip of the delta'd utterance and reads its frames t - left ..
//   t + right, so the tile needs the delta'd frames u0 .. u0 + S, u0 = r0 skip - left, S = (rows - 1) skip + left + 1 + right, and those the
//   base frames v0 .. v0 + S + 2 ow, v0 = u0 - ow, ow = order window (the reach of the widest delta filter).
//   1. The base frames of that span that lie in [0, T_b) are ONE contiguous run of the padded batch: copied to LDS with consecutive lanes on
//      consecutive floats.  Nothing at or beyond frames[b] is read; a clamped index always lies between two indices of the span, so it is
//      in LDS.
//   2. With deltas, every delta'd frame of the span is formed once (not once per spliced copy): [static | d | dd], each element the ascending
//      float64 sum over the filter's offsets, rounded once.  Without, the staged base frames ARE the delta'd frames.
//   3. Every output row is written from LDS, lane after lane on consecutive floats of the row: left + 1 + right runs of F1 floats.
//   Rows from the utterance's kept count on -- the downsample pad and whatever lies behind n_out up to Tout_max -- are written as zeros.
#include <algorithm>

#include "common.h"

namespace {

constexpr int CONTEXT_TILE_ROWS = 16;              // output rows per workgroup where the span fits CONTEXT_LDS_WORDS
constexpr int CONTEXT_LDS_WORDS = 16384;           // 64 KB: the budget the tile is sized for (several workgroups per CU at the recipe's sizes)
constexpr int CONTEXT_LDS_WORDS_ONE = 36864;       // 144 KB of the CU's 160: what a single output row's span may take
constexpr int CONTEXT_MAX_CTX = 64;                // left, right
constexpr int CONTEXT_MAX_SKIP = 1024;             // skip, n_downsample
constexpr int CONTEXT_MAX_WINDOW = 5;
constexpr int CONTEXT_MAX_ORDER = 2;
constexpr int CONTEXT_MAX_DIM = 1 << 16;           // F
constexpr int CONTEXT_MAX_FRAMES = 1 << 30;
constexpr int CONTEXT_SCALES = 2 * CONTEXT_MAX_ORDER * CONTEXT_MAX_WINDOW + 1;   // 21: the longest filter

struct ContextGeom {
  int left, right, skip, nd, order, window;        // skip >= 1 here
  int ow, F, F1, F2, rows;
  size_t words;                                    // LDS words of a full tile
};

static inline long long context_words(const ContextGeom &g, int rows) {
  const long long S = (long long)(rows - 1) * g.skip + g.left + 1 + g.right;
  return g.order ? (S + 2 * g.ow) * g.F + S * g.F1 : S * g.F;
}

static int context_geom(const ctcn_context_opts *o, int F, ContextGeom *g, const char **why) {
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (o->left < 0 || o->right < 0 || o->skip < 0 || o->n_downsample < 1 || o->delta_order < 0 || o->delta_window < 1 || F < 1) {
    *why = "left, right, skip and delta_order must not be negative; n_downsample, delta_window and F must be positive";
    return CTCN_EINVAL;
  }
  if (o->left > CONTEXT_MAX_CTX || o->right > CONTEXT_MAX_CTX) { *why = "more than 64 context frames on a side"; return CTCN_EUNSUPPORTED; }
  if (o->skip > CONTEXT_MAX_SKIP || o->n_downsample > CONTEXT_MAX_SKIP) { *why = "skip or n_downsample beyond 1024"; return CTCN_EUNSUPPORTED; }
  if (o->delta_order > CONTEXT_MAX_ORDER) { *why = "delta_order beyond 2"; return CTCN_EUNSUPPORTED; }
  if (o->delta_window > CONTEXT_MAX_WINDOW) { *why = "delta_window beyond 5"; return CTCN_EUNSUPPORTED; }
  if (F > CONTEXT_MAX_DIM) { *why = "more than 65 536 columns"; return CTCN_EUNSUPPORTED; }
  g->left = o->left; g->right = o->right; g->skip = std::max(o->skip, 1); g->nd = o->n_downsample; g->order = o->delta_order;
  g->window = o->delta_window; g->ow = g->order * g->window; g->F = F; g->F1 = F * (g->order + 1); g->F2 = (g->left + 1 + g->right) * g->F1;
  int rows = CONTEXT_TILE_ROWS;
  while (rows > 1 && context_words(*g, rows) > CONTEXT_LDS_WORDS) --rows;
  if (context_words(*g, rows) > (rows > 1 ? CONTEXT_LDS_WORDS : CONTEXT_LDS_WORDS_ONE)) {
    *why = "the frames behind a single output row do not fit the LDS";
    return CTCN_EUNSUPPORTED;
  }
  g->rows = rows;
  g->words = (size_t)context_words(*g, rows);
  return CTCN_OK;
}

// kept rows and output rows of an utterance of T frames (T >= 0, skip >= 1)
static inline int context_kept(int T, int skip) { return (int)(((long long)T + skip - 1) / skip); }
static inline long long context_out(int T, int skip, int nd) { return ((long long)context_kept(T, skip) + nd - 1) / nd * nd; }

// Kaldi's DeltaFeatures scales in float32: s0 = [1]; s_i[j + k + window] += j * s_{i-1}[k], j in [-window, window]; s_i /= sum j^2.
// Row i of `scales` (stride CONTEXT_SCALES) holds the 2 i window + 1 values of order i.
static void delta_scales(int order, int window, float *scales) {
#pragma clang fp contract(off)                                        // Kaldi's float32 multiply, then add: a fused one changes the last bit
  for (int i = 0; i <= order; ++i)
    for (int k = 0; k < CONTEXT_SCALES; ++k) scales[i * CONTEXT_SCALES + k] = 0.f;
  scales[0] = 1.f;
  for (int i = 1; i <= order; ++i) {
    const float *prev = scales + (i - 1) * CONTEXT_SCALES;
    float *cur = scales + i * CONTEXT_SCALES;
    const int prev_offset = (i - 1) * window, cur_offset = i * window;
    float normalizer = 0.f;
    for (int j = -window; j <= window; ++j) {
      normalizer += (float)(j * j);
      for (int k = -prev_offset; k <= prev_offset; ++k) cur[j + k + cur_offset] += (float)j * prev[k + prev_offset];
    }
    const float inv = (float)(1.0 / (double)normalizer);              // Kaldi's cur_scales.Scale(1.0 / normalizer)
    for (int k = 0; k < 2 * cur_offset + 1; ++k) cur[k] *= inv;
  }
}

struct ContextArgs {
  const float *feats;
  const int32_t *frames;
  float *out;
  int32_t *out_frames;
  float *fractions;
  int Tin_max, Tout_max, F, F1, F2, left, right, skip, nd, order, window, rows;
  float s1[2 * CONTEXT_MAX_WINDOW + 1], s2[CONTEXT_SCALES];
};

__global__ __launch_bounds__(256) void frame_context_kernel(ContextArgs a) {
  extern __shared__ __align__(16) float smem_f[];
  __shared__ float sc[2][CONTEXT_SCALES];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int F = a.F, F1 = a.F1, F2 = a.F2, skip = a.skip;
  const int T = min(max(a.frames[b], 0), a.Tin_max);
  const int kept = (int)(((long long)T + skip - 1) / skip);
  const int n_out = (int)(((long long)kept + a.nd - 1) / a.nd * a.nd);
  if (blockIdx.x == 0 && tid == 0) {
    a.out_frames[b] = n_out;
    a.fractions[b] = a.Tout_max > 0 ? (float)((double)n_out / (double)a.Tout_max) : 0.f;
  }
  const int r0 = blockIdx.x * a.rows;
  const int nrows = min(a.rows, a.Tout_max - r0);                      // rows of this tile inside the batch
  if (nrows <= 0) return;
  const int nk = min(max(kept - r0, 0), nrows);                        // those of them that carry frames
  float *out = a.out + ((size_t)b * a.Tout_max + r0) * F2;
  for (size_t i = (size_t)nk * F2 + tid; i < (size_t)nrows * F2; i += 256) out[i] = 0.f;
  if (nk <= 0) return;                                                 // (the whole workgroup)

  const int ow = a.order * a.window;
  const int S = (nk - 1) * skip + a.left + 1 + a.right;                // delta'd frames u0 .. u0 + S
  const int u0 = r0 * skip - a.left, v0 = u0 - ow;
  float *raw = smem_f;                                                 // base frames v0 .. v0 + S + 2 ow, F floats each
  float *dl = a.order ? smem_f + (size_t)(a.rows - 1) * skip * F + (size_t)(a.left + 1 + a.right + 2 * ow) * F : smem_f;   // F1 floats each
  {
    const int lo = max(v0, 0), hi = min(v0 + S + 2 * ow, T);           // hi > lo: frame r0 skip < T lies in the span
    const float *src = a.feats + ((size_t)b * a.Tin_max + lo) * F;
    float *dst = raw + (size_t)(lo - v0) * F;
    const int n = (hi - lo) * F;
    for (int i = tid; i < n; i += 256) dst[i] = src[i];
  }
  if (a.order) {
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < 2 * CONTEXT_MAX_WINDOW + 1; ++k) sc[0][k] = a.s1[k];
#pragma unroll
      for (int k = 0; k < CONTEXT_SCALES; ++k) sc[1][k] = a.s2[k];
    }
    __syncthreads();
    const int ulo = max(u0, 0), uhi = min(u0 + S, T);
    const int n = (uhi - ulo) * F;
    for (int i = tid; i < n; i += 256) {
      const int du = i / F, f = i - du * F;
      const int u = ulo + du;
      float *d = dl + (size_t)(u - u0) * F1 + f;
      d[0] = raw[(size_t)(u - v0) * F + f];
      for (int o = 1; o <= a.order; ++o) {
        const int reach = o * a.window;
        const float *s = sc[o - 1];
        double acc = 0.0;
        for (int j = -reach; j <= reach; ++j) {                        // ascending offsets: a function of the utterance alone
          const float w = s[j + reach];
          if (w != 0.f) acc += (double)w * (double)raw[(size_t)(min(max(u + j, 0), T - 1) - v0) * F + f];
        }
        d[o * F] = (float)acc;
      }
    }
  }
  __syncthreads();

  const int n = nk * F2;
  for (int i = tid; i < n; i += 256) {
    const int r = i / F2, e = i - r * F2;
    const int c = e / F1, f = e - c * F1;
    const int u = min(max((r0 + r) * skip - a.left + c, 0), T - 1);
    out[i] = dl[(size_t)(u - u0) * F1 + f];
  }
}

}  // namespace

extern "C" int ctcn_context_frames(int num_frames, int skip, int n_downsample) {
  CTCN_REQUIRE(num_frames >= 0 && skip >= 0 && n_downsample >= 1, "ctcn_context_frames: bad args (frames %d, skip %d, n_downsample %d)", num_frames,
               skip, n_downsample);
  const long long n = context_out(num_frames, std::max(skip, 1), n_downsample);
  if (n > 0x7fffffffLL) { ctcn_set_error("ctcn_context_frames: %lld output frames, beyond int", n); return CTCN_EUNSUPPORTED; }
  return (int)n;
}

extern "C" int ctcn_delta_scales(int order, int window, float *scales) {
  CTCN_REQUIRE(scales && order >= 0 && window >= 1, "ctcn_delta_scales: bad args (order %d, window %d)", order, window);
  if (order > CONTEXT_MAX_ORDER || window > CONTEXT_MAX_WINDOW) {
    ctcn_set_error("ctcn_delta_scales: order %d beyond 2 or window %d beyond 5", order, window);
    return CTCN_EUNSUPPORTED;
  }
  float tab[(CONTEXT_MAX_ORDER + 1) * CONTEXT_SCALES];
  delta_scales(order, window, tab);
  memcpy(scales, tab + order * CONTEXT_SCALES, sizeof(float) * (2 * order * window + 1));
  return 2 * order * window + 1;
}

extern "C" int ctcn_frame_context_tile(const ctcn_context_opts *opts, int F) {
  ContextGeom g;
  const char *why;
  const int rc = context_geom(opts, F, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_frame_context_tile: %s", why); return rc; }
  return g.rows;
}

extern "C" int ctcn_frame_context(const float *feats, const int32_t *frames, const ctcn_context_opts *opts, float *out, int32_t *out_frames,
                                  float *fractions, int B, int Tin_max, int F, int Tout_max, void *stream) {
  ContextGeom g;
  const char *why;
  const int rc = context_geom(opts, F, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_frame_context: %s", why); return rc; }
  CTCN_REQUIRE(frames && out_frames && fractions && B > 0 && B <= 65535 && Tin_max >= 0 && Tin_max <= CONTEXT_MAX_FRAMES &&
                   (feats || Tin_max == 0) && (out || Tout_max == 0),
               "ctcn_frame_context: bad args (B %d at most 65 535, Tin_max %d at most 2^30)", B, Tin_max);
  CTCN_REQUIRE((long long)Tout_max == context_out(Tin_max, g.skip, g.nd), "ctcn_frame_context: Tout_max %d is not ctcn_context_frames(%d) = %lld",
               Tout_max, Tin_max, context_out(Tin_max, g.skip, g.nd));
  ContextArgs a;
  a.feats = feats; a.frames = frames; a.out = out; a.out_frames = out_frames; a.fractions = fractions;
  a.Tin_max = Tin_max; a.Tout_max = Tout_max; a.F = F; a.F1 = g.F1; a.F2 = g.F2; a.left = g.left; a.right = g.right; a.skip = g.skip; a.nd = g.nd;
  a.order = g.order; a.window = g.window; a.rows = g.rows;
  float tab[(CONTEXT_MAX_ORDER + 1) * CONTEXT_SCALES];
  delta_scales(g.order, g.window, tab);
  for (int k = 0; k < 2 * CONTEXT_MAX_WINDOW + 1; ++k) a.s1[k] = g.order >= 1 ? tab[CONTEXT_SCALES + k] : 0.f;
  for (int k = 0; k < CONTEXT_SCALES; ++k) a.s2[k] = g.order >= 2 ? tab[2 * CONTEXT_SCALES + k] : 0.f;
  const size_t lds = g.words * 4;
  const dim3 grid(std::max(ceil_div(Tout_max, g.rows), 1), B);
  if (lds > 64 * 1024)
    CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(frame_context_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(frame_context_kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_frame_context_host(const float *feats, int num_frames, int F, const ctcn_context_opts *opts, float *out, int out_rows,
                                       float *fraction) {
  ContextGeom g;
  const char *why;
  const int rc = context_geom(opts, F, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_frame_context_host: %s", why); return rc; }
  CTCN_REQUIRE(num_frames >= 0 && num_frames <= CONTEXT_MAX_FRAMES && out_rows >= 0 && (feats || num_frames == 0) && (out || out_rows == 0),
               "ctcn_frame_context_host: bad args");
  const int T = num_frames, kept = context_kept(T, g.skip);
  const long long n_out = context_out(T, g.skip, g.nd);
  CTCN_REQUIRE(n_out <= out_rows, "ctcn_frame_context_host: %lld output rows, room for %d", n_out, out_rows);
  float tab[(CONTEXT_MAX_ORDER + 1) * CONTEXT_SCALES];
  delta_scales(g.order, g.window, tab);
  for (int r = 0; r < kept; ++r) {
    float *orow = out + (size_t)r * g.F2;
    for (int c = 0; c < g.left + 1 + g.right; ++c) {
      const int u = std::min(std::max(r * g.skip - g.left + c, 0), T - 1);
      float *dst = orow + (size_t)c * g.F1;
      for (int f = 0; f < F; ++f) dst[f] = feats[(size_t)u * F + f];
      for (int o = 1; o <= g.order; ++o) {
        const int reach = o * g.window;
        const float *s = tab + o * CONTEXT_SCALES;
        for (int f = 0; f < F; ++f) {
          double acc = 0.0;
          for (int j = -reach; j <= reach; ++j) {
            const float w = s[j + reach];
            if (w != 0.f) acc += (double)w * (double)feats[(size_t)std::min(std::max(u + j, 0), T - 1) * F + f];
          }
          dst[o * F + f] = (float)acc;
        }
      }
    }
  }
  for (size_t i = (size_t)kept * g.F2; i < (size_t)out_rows * g.F2; ++i) out[i] = 0.f;
  if (fraction) *fraction = out_rows > 0 ? (float)((double)n_out / (double)out_rows) : 0.f;
  return (int)n_out;
}
