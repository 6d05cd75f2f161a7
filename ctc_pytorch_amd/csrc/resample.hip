// resample.hip -- waveform resampling in front of the feature kernels: Kaldi's LinearResample as ResampleWaveform configures it, a polyphase
// windowed-sinc filter (ctcn_resample_samples, ctcn_resample_plan_bytes, ctcn_resample_plan, ctcn_resample; ctcn_resample_host, the same sum
// on the host; the computation and the plan layout in include/ctcn.h).  Speed perturbation by f is the same call with fin = round(rate f).
//
// resample_kernel: grid (output tiles, utterances), four waves per workgroup.
//   A tile is `upt` whole units of `ou` outputs (ou = fout / gcd: the number of filter phases), so its first input sample is the integer
//   tile * upt * iu + first[0] and the phase of an output is its local index mod ou.
//   1. The workgroup stages first | ntaps | the weight table (row stride odd: lanes on neighbouring phases fall on different LDS banks) and
//      the tile's input span -- (upt - 1) iu + the reach of one unit's taps -- as float32 (int16 converted here).  Positions outside [0, n)
//      are zero by select: whatever lies behind an utterance in the padded row is never read.
//   2. Every lane computes whole outputs tid, tid + 256, ...: the ascending sum over the phase's taps in float64 (a float32 x float32
//      product is exact there, so the sum is the same number with or without contraction), rounded once.  No cross-lane reduction; the
//      stores of a wave are 64 consecutive floats.
//   Outputs of the tile from the utterance's count on (and behind it up to Mmax) are written as zeros first.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.h"

namespace {

constexpr int RESAMPLE_TABLE_WORDS = 24576;        // ou x stride floats of the weight table in LDS: 96 KB of the CU's 160
constexpr int RESAMPLE_SPAN_WORDS = 8192;          // the staged input span of a tile: 32 KB
constexpr int RESAMPLE_TILE = 2048;                // outputs per workgroup, rounded down to whole units (one unit where ou is larger)
constexpr int RESAMPLE_HEADER = 8;                 // words in front of first[]
constexpr int RESAMPLE_MAX_RATE = 1 << 24;

struct ResampleGeom {
  int fin, fout, iu, ou, nz;
  double cutoff, ww;
  int maxtaps, stride, min_first, extent;          // extent: max (first + ntaps) - min first, the reach of one unit's taps
  int upt, tile, span;                             // units and outputs per tile, staged samples per tile
  size_t words;
};

static inline void resample_phase(const ResampleGeom &g, int i, int *lo, int *hi) {
  const double t_out = (double)i / g.fout;
  *lo = (int)ceil((t_out - g.ww) * g.fin);
  *hi = (int)floor((t_out + g.ww) * g.fin);
}

static int resample_geom(const ctcn_resample_opts *o, ResampleGeom *g, const char **why) {
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (o->orig_freq <= 0 || o->new_freq <= 0) { *why = "sample rates must be positive"; return CTCN_EUNSUPPORTED; }
  if (o->orig_freq > RESAMPLE_MAX_RATE || o->new_freq > RESAMPLE_MAX_RATE) { *why = "sample rates beyond 2^24 Hz"; return CTCN_EUNSUPPORTED; }
  if (o->num_zeros <= 0) { *why = "num_zeros must be positive"; return CTCN_EUNSUPPORTED; }
  if (!(o->cutoff > 0.0)) { *why = "cutoff must be positive"; return CTCN_EUNSUPPORTED; }
  if (o->cutoff * 2 > std::min(o->orig_freq, o->new_freq)) { *why = "cutoff above the Nyquist frequency of the lower rate"; return CTCN_EUNSUPPORTED; }
  g->fin = o->orig_freq; g->fout = o->new_freq; g->nz = o->num_zeros; g->cutoff = o->cutoff;
  const int gc = std::gcd(g->fin, g->fout);
  g->iu = g->fin / gc; g->ou = g->fout / gc;
  g->ww = g->nz / (2 * g->cutoff);
  if (g->ou > RESAMPLE_TABLE_WORDS || 2.0 * g->ww * g->fin + 2 > RESAMPLE_TABLE_WORDS) { *why = "filter table beyond the LDS budget"; return CTCN_EUNSUPPORTED; }
  int maxtaps = 0, min_first = 0x7fffffff, max_end = -0x7fffffff;
  for (int i = 0; i < g->ou; ++i) {
    int lo, hi;
    resample_phase(*g, i, &lo, &hi);
    maxtaps = std::max(maxtaps, hi - lo + 1);
    min_first = std::min(min_first, lo);
    max_end = std::max(max_end, hi + 1);
  }
  if (maxtaps < 1) { *why = "empty filter"; return CTCN_EUNSUPPORTED; }
  g->maxtaps = maxtaps; g->stride = maxtaps | 1; g->min_first = min_first; g->extent = max_end - min_first;
  if ((long long)g->ou * g->stride > RESAMPLE_TABLE_WORDS) { *why = "filter table beyond the LDS budget"; return CTCN_EUNSUPPORTED; }
  if (g->extent > RESAMPLE_SPAN_WORDS) { *why = "one unit of input samples beyond the LDS budget"; return CTCN_EUNSUPPORTED; }
  g->upt = std::max(1, std::min(RESAMPLE_TILE / g->ou, (RESAMPLE_SPAN_WORDS - g->extent) / g->iu + 1));
  g->tile = g->upt * g->ou;
  g->span = (g->upt - 1) * g->iu + g->extent;
  g->words = (size_t)RESAMPLE_HEADER + 2 * (size_t)g->ou + (size_t)g->ou * g->stride;
  return CTCN_OK;
}

static inline long long resample_count(long long n, int fin, int fout) { return n <= 0 ? 0 : (n * fout + fin - 1) / fin; }

struct ResampleArgs {
  const void *wave;
  const int32_t *lens;
  const int32_t *plan;                             // behind the header: first | ntaps | weights
  float *out;
  int is_i16, Nmax, Mmax, fin, fout, iu, ou, stride, upt, min_first, extent;
};

__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
  extern __shared__ __align__(16) int smem_i[];
  const int ou = a.ou, iu = a.iu, stride = a.stride;
  int *first = smem_i, *ntaps = smem_i + ou;
  float *wts = reinterpret_cast<float *>(smem_i + 2 * ou);
  float *span = wts + ou * stride;

  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const long long m = min(((long long)n * a.fout + a.fin - 1) / a.fin, (long long)a.Mmax);
  const int tile = a.upt * ou;
  const long long k0 = (long long)blockIdx.x * tile;
  const int kend = (int)min((long long)tile, a.Mmax - k0);            // outputs of this tile inside the row
  const int nk = (int)min(max(m - k0, 0LL), (long long)kend);         // those of them the utterance has
  float *out = a.out + (size_t)b * a.Mmax + k0;
  for (int i = nk + tid; i < kend; i += 256) out[i] = 0.f;
  if (nk <= 0) return;                                                // (the whole workgroup)

  for (int i = tid; i < 2 * ou + ou * stride; i += 256) smem_i[i] = a.plan[i];
  {
    const int units = (nk + ou - 1) / ou;
    const int span_len = (units - 1) * iu + a.extent;
    const long long s0 = (long long)blockIdx.x * a.upt * iu + a.min_first;
    const size_t base = (size_t)b * a.Nmax;
    for (int i = tid; i < span_len; i += 256) {
      const long long s = s0 + i;
      float v = 0.f;
      if (s >= 0 && s < n) v = wave_sample(a.wave, a.is_i16, base + s);
      span[i] = v;
    }
  }
  __syncthreads();

  for (int k = tid; k < nk; k += 256) {
    const int u = k / ou, p = k - u * ou;
    const float *w = wts + p * stride;
    const float *x = span + (first[p] - a.min_first + u * iu);
    const int nt = ntaps[p];
    double acc = 0.0;
    for (int j = 0; j < nt; ++j) acc += (double)w[j] * (double)x[j];    // ascending taps: a function of the utterance alone
    out[k] = (float)acc;
  }
}

}  // namespace

extern "C" int ctcn_resample_samples(long long num_samples, int orig_freq, int new_freq) {
  CTCN_REQUIRE(num_samples >= 0 && orig_freq > 0 && new_freq > 0 && orig_freq <= RESAMPLE_MAX_RATE && new_freq <= RESAMPLE_MAX_RATE &&
                   num_samples < (1LL << 38),
               "ctcn_resample_samples: bad args (samples %lld, rates %d -> %d)", num_samples, orig_freq, new_freq);
  const long long m = resample_count(num_samples, orig_freq, new_freq);
  if (m > 0x7fffffffLL) { ctcn_set_error("ctcn_resample_samples: %lld output samples, beyond int", m); return CTCN_EUNSUPPORTED; }
  return (int)m;
}

extern "C" size_t ctcn_resample_plan_bytes(const ctcn_resample_opts *opts) {
  ResampleGeom g;
  const char *why;
  return resample_geom(opts, &g, &why) == CTCN_OK ? g.words * 4 : 0;
}

extern "C" int ctcn_resample_plan(const ctcn_resample_opts *opts, void *plan, size_t plan_bytes) {
  ResampleGeom g;
  const char *why;
  const int rc = resample_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_resample_plan: %s", why); return rc; }
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4, "ctcn_resample_plan: buffer of %zu bytes needed", g.words * 4);
  const double two_pi = 6.283185307179586476925286766559, pi = 3.14159265358979323846264338327950288;
  int32_t *hdr = static_cast<int32_t *>(plan), *first = hdr + RESAMPLE_HEADER, *ntaps = first + g.ou;
  float *wts = reinterpret_cast<float *>(ntaps + g.ou);
  hdr[0] = g.ou; hdr[1] = g.iu; hdr[2] = g.stride; hdr[3] = g.maxtaps; hdr[4] = g.tile; hdr[5] = g.min_first; hdr[6] = g.span; hdr[7] = 0;
  for (int i = 0; i < g.ou; ++i) {
    int lo, hi;
    resample_phase(g, i, &lo, &hi);
    const double t_out = (double)i / g.fout;
    first[i] = lo;
    ntaps[i] = hi - lo + 1;
    float *w = wts + (size_t)i * g.stride;
    for (int j = 0; j < g.stride; ++j) {
      if (j > hi - lo) { w[j] = 0.f; continue; }
      const double dt = (double)(lo + j) / g.fin - t_out;
      const double win = fabs(dt) < g.ww ? 0.5 * (1 + cos(two_pi * g.cutoff / g.nz * dt)) : 0.0;
      const double filt = dt != 0.0 ? sin(two_pi * g.cutoff * dt) / (pi * dt) : 2 * g.cutoff;
      w[j] = (float)(filt * win / g.fin);
    }
  }
  return CTCN_OK;
}

extern "C" int ctcn_resample(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_resample_opts *opts, const void *plan, float *out,
                             int B, int Nmax, int Mmax, void *stream) {
  ResampleGeom g;
  const char *why;
  const int rc = resample_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_resample: %s", why); return rc; }
  CTCN_REQUIRE(lens && plan && B > 0 && B <= 65535 && Nmax >= 0 && Mmax >= 0 && (wave || Nmax == 0) && (out || Mmax == 0),
               "ctcn_resample: bad args (B %d at most 65 535)", B);
  ResampleArgs a;
  a.wave = wave; a.lens = lens; a.plan = static_cast<const int32_t *>(plan) + RESAMPLE_HEADER; a.out = out;
  a.is_i16 = wave_is_int16 != 0; a.Nmax = Nmax; a.Mmax = Mmax; a.fin = g.fin; a.fout = g.fout; a.iu = g.iu; a.ou = g.ou; a.stride = g.stride;
  a.upt = g.upt; a.min_first = g.min_first; a.extent = g.extent;
  const size_t lds = (2 * (size_t)g.ou + (size_t)g.ou * g.stride + g.span) * 4;
  const dim3 grid(std::max(ceil_div(Mmax, g.tile), 1), B);
  if (lds > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(resample_kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_resample_host(const void *wave, int wave_is_int16, int num_samples, const ctcn_resample_opts *opts, const void *plan, float *out,
                                  int out_cap) {
  ResampleGeom g;
  const char *why;
  const int rc = resample_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_resample_host: %s", why); return rc; }
  CTCN_REQUIRE(plan && num_samples >= 0 && out_cap >= 0 && (wave || num_samples == 0) && (out || out_cap == 0), "ctcn_resample_host: bad args");
  const int32_t *hdr = static_cast<const int32_t *>(plan), *first = hdr + RESAMPLE_HEADER, *ntaps = first + g.ou;
  CTCN_REQUIRE(hdr[0] == g.ou && hdr[1] == g.iu && hdr[2] == g.stride, "ctcn_resample_host: the plan is not the one of these options");
  const float *wts = reinterpret_cast<const float *>(ntaps + g.ou);
  const long long m = resample_count(num_samples, g.fin, g.fout);
  CTCN_REQUIRE(m <= out_cap, "ctcn_resample_host: %lld output samples, room for %d", m, out_cap);
  for (long long k = 0; k < m; ++k) {
    const long long u = k / g.ou;
    const int p = (int)(k - u * g.ou);
    const float *w = wts + (size_t)p * g.stride;
    const long long s0 = first[p] + u * g.iu;
    double acc = 0.0;
    for (int j = 0; j < ntaps[p]; ++j) {
      const long long s = s0 + j;
      float v = 0.f;
      if (s >= 0 && s < num_samples) v = wave_sample(wave, wave_is_int16, s);
      acc += (double)w[j] * (double)v;
    }
    out[k] = (float)acc;
  }
  return (int)m;
}
