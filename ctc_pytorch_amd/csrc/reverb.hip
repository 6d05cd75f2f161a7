// reverb.hip -- multi-condition data on the waveform, the stage in front of resampling's consumers: a room impulse response convolved into
// every utterance and background noise added at a drawn signal-to-noise ratio, what Kaldi's wav-reverberate does under
// --shift-output=false --normalize-output=true (ctcn_reverb_bank_bytes, ctcn_reverb_bank: the bank block on the host; ctcn_reverb_plan: the
// draws of one utterance; ctcn_reverb_ws_bytes, ctcn_reverb: the device call; ctcn_reverb_host: the same computation for one utterance on
// the host; ctcn_reverb_limits: the constants below; the computation step by step in include/ctcn.h).
//
// The launch chain of ctcn_reverb, every launch on the caller's stream, a launch boundary wherever a sum over a whole utterance is needed:
//   1. reverb_conv_kernel, grid (output tiles + early-window tiles, utterances), four waves per workgroup.  A tile is REVERB_TILE outputs,
//      every lane owns REVERB_RUN consecutive ones.  Taps are walked in chunks of REVERB_TAP_CHUNK, ascending: the workgroup stages the
//      chunk as float64 and the tile's input span (tile + chunk - 1 samples, zeros outside [0, n) by select, int16 converted here) in LDS;
//      a lane then reads eight taps (broadcast) and eight new samples per 64 float64 FMAs, the input window sliding through its
//      registers (two runs of eight samples that swap roles from one group of eight taps to the next: nothing is moved).  The tile's outputs go back through LDS so that stores are consecutive per wave and the power sums of x^2 and y^2 take
//      the contract's shape.  Early-window tiles run the same code over h[lo, hi) and keep only their power sums: the early signal is
//      never stored.  An utterance without an RIR is copied.  Elements [n, Nmax) are written as zeros here.
//   2. reverb_stats_kernel (stage 0), one wave per utterance: P_in, P_sig and the gain g from the partial sums, added in ascending order;
//      where no noise launch follows, the scale s as well.
//   3. reverb_mix_kernel: z = y + g q, in place, with the partial sums of z^2.           (only where a noise draw can be on)
//   4. reverb_stats_kernel (stage 1): s from P_in and the sums of z^2.                    (only with 3. and normalize)
//   5. reverb_scale_kernel: out = s z, in place.                                         (only with normalize)
// No atomics, no grid-wide barrier, no flag: a partial sum has one writer and is read after a launch boundary.
// The host entry points run the same reverb_draw / reverb_gain / reverb_mix / reverb_norm / reverb_scale: one definition of the arithmetic.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace {

// The constants of the contract and of the kernel's shape, in one place (ctcn_reverb_limits hands them out).
constexpr int REVERB_POW_CHUNK = 1024;             // elements per chunk of the power sum S(v): the halving tree starts at +512
constexpr int REVERB_TILE = 2048;                  // outputs per workgroup: two power-sum chunks
constexpr int REVERB_RUN = 8;                      // consecutive outputs per lane
constexpr int REVERB_TAP_CHUNK = 1024;             // taps staged at a time
constexpr int REVERB_MAX_TAPS = 16384;             // K
constexpr int REVERB_MAX_SNRS = 16;
constexpr int REVERB_MAX_SAMPLES = 1 << 30;        // n, L
constexpr int REVERB_HEADER = 16;                  // int32 words in front of the bank's tables
constexpr int REVERB_MAGIC = 0x52564231;           // "RVB1"
constexpr int REVERB_STATS = 8;                    // doubles per utterance: P_in, P_sig, g, s, apply (0 / 1), spare
static_assert(REVERB_TILE == 256 * REVERB_RUN && REVERB_TILE == 2 * REVERB_POW_CHUNK && REVERB_POW_CHUNK == 4 * 256 && REVERB_TAP_CHUNK % 8 == 0,
              "the kernels' index arithmetic");

// The bank block as a set of pointers: the header is read on the host, the tables lie behind `base` (the host block or its device copy).
struct ReverbBank {
  int R, N, J, kstride, lstride, emax;
  const int32_t *rir_meta;                         // R x (K, p, lo, hi)
  const int32_t *noise_len;                        // N
  const double *pm, *gj;                           // N, REVERB_MAX_SNRS
  const float *rirs, *noises;                      // R x kstride, N x lstride
};

static bool reverb_view(const void *host_block, const void *base, ReverbBank *bk) {
  const int32_t *h = static_cast<const int32_t *>(host_block);
  if (!h || !base || h[0] != REVERB_MAGIC) return false;
  const int32_t *w = static_cast<const int32_t *>(base);
  bk->R = h[1]; bk->N = h[2]; bk->J = h[3]; bk->kstride = h[4]; bk->lstride = h[5]; bk->emax = h[6];
  bk->rir_meta = w + h[8];
  bk->noise_len = w + h[9];
  bk->pm = reinterpret_cast<const double *>(w + h[10]);
  bk->gj = bk->pm + bk->N;
  bk->rirs = reinterpret_cast<const float *>(w) + (size_t)(uint32_t)h[11];
  bk->noises = bk->rirs + (size_t)bk->R * bk->kstride;
  return true;
}

// Offsets (in 4-byte words) of the tables behind the header; the doubles start on an 8-byte boundary.
struct ReverbLayout { size_t meta, nlen, dbl, rirs, words; };
static ReverbLayout reverb_layout(int R, int kstride, int N, int lstride) {
  ReverbLayout l;
  l.meta = REVERB_HEADER;
  l.nlen = l.meta + 4 * (size_t)R;
  l.dbl = align_up(l.nlen + (size_t)N, 2);
  l.rirs = l.dbl + 2 * ((size_t)N + REVERB_MAX_SNRS);
  l.words = l.rirs + (size_t)R * kstride + (size_t)N * lstride;
  return l;
}

static int reverb_shape_check(int R, int kstride, int N, int lstride, int J, const char **why) {
  if (R < 0 || N < 0 || J < 0 || kstride < 0 || lstride < 0) { *why = "negative count"; return CTCN_EINVAL; }
  if (R == 0 && N == 0) { *why = "both banks are empty"; return CTCN_EINVAL; }
  if ((R > 0 && kstride < 1) || (N > 0 && lstride < 1)) { *why = "a bank with rows of no elements"; return CTCN_EINVAL; }
  if (N > 0 && J < 1) { *why = "a noise bank needs at least one SNR"; return CTCN_EINVAL; }
  if (J > REVERB_MAX_SNRS) { *why = "more than 16 SNRs"; return CTCN_EUNSUPPORTED; }
  if (R > 0 && kstride > REVERB_MAX_TAPS) { *why = "an impulse response of more than 16 384 taps"; return CTCN_EUNSUPPORTED; }
  if (N > 0 && lstride > REVERB_MAX_SAMPLES) { *why = "a noise row of more than 2^30 samples"; return CTCN_EUNSUPPORTED; }
  if (R > (1 << 20) || N > (1 << 20)) { *why = "more than 2^20 rows in a bank"; return CTCN_EUNSUPPORTED; }
  if (reverb_layout(R, kstride, N, lstride).words > 0x7fffffffull) { *why = "a bank beyond 2^31 words"; return CTCN_EUNSUPPORTED; }
  return CTCN_OK;
}

static int reverb_opts_check(const ctcn_reverb_opts *o, const char **why) {
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (!(o->rir_prob >= 0.f && o->rir_prob <= 1.f) || !(o->noise_prob >= 0.f && o->noise_prob <= 1.f)) {
    *why = "a probability outside [0, 1]";
    return CTCN_EINVAL;
  }
  return CTCN_OK;
}

// floor(prob 2^24): the draw is on where rnd(word, 2^24) lies below it.
static uint32_t reverb_threshold(float prob) { return (uint32_t)floor((double)prob * 16777216.0); }

__host__ __device__ __forceinline__ int reverb_cdiv(int a, int b) { return (a + b - 1) / b; }

__host__ __device__ __forceinline__ int reverb_rnd(uint32_t word, int n) { return (int)(((uint64_t)(word >> 8) * (uint64_t)(uint32_t)n) >> 24); }

// The draws of utterance u: r and m are -1 where that part is off; j and off are 0 without a noise row.
struct ReverbDraw { int r, m, j, off; };
__host__ __device__ inline ReverbDraw reverb_draw(const ReverbBank &bk, uint32_t rir_thr, uint32_t noise_thr, uint64_t seed, uint64_t u) {
  ReverbDraw d = {-1, -1, 0, 0};
  uint32_t w[4];
  if (bk.R > 0 && rir_thr > 0) {
    philox4(seed, (u << 8) | 0u, w);
    if ((uint32_t)reverb_rnd(w[0], 1 << 24) < rir_thr) d.r = reverb_rnd(w[1], bk.R);
  }
  if (bk.N > 0 && noise_thr > 0) {
    philox4(seed, (u << 8) | 1u, w);
    if ((uint32_t)reverb_rnd(w[0], 1 << 24) < noise_thr) {
      d.m = reverb_rnd(w[1], bk.N);
      d.j = reverb_rnd(w[2], bk.J);
      d.off = reverb_rnd(w[3], bk.noise_len[d.m]);
    }
  }
  return d;
}

__host__ __device__ __forceinline__ double reverb_sqrt(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(v);
#else
  return sqrt(v);
#endif
}

// g = sqrt((G P_sig) / P_m) and z = fl32(y + g q): every float64 operation rounded on its own.
__host__ __device__ __forceinline__ double reverb_gain(double G, double p_sig, double p_m) {
#pragma clang fp contract(off)
  const double num = G * p_sig;
  const double ratio = num / p_m;
  return reverb_sqrt(ratio);
}
__host__ __device__ __forceinline__ float reverb_mix(float y, double g, float q) {
#pragma clang fp contract(off)
  const double t = g * (double)q;
  return (float)((double)y + t);
}
__host__ __device__ __forceinline__ double reverb_norm(double p_in, double p_out) {
#pragma clang fp contract(off)
  const double ratio = p_in / p_out;
  return reverb_sqrt(ratio);
}
__host__ __device__ __forceinline__ float reverb_scale(double s, float z) { return (float)(s * (double)z); }

// ---- the device side ------------------------------------------------------------------------------------------------------------------

struct ReverbArgs {
  const void *wave;
  const int32_t *lens;
  float *out;
  double *px, *py, *pz, *pe, *stats;               // partial sums per power chunk (B x cy, B x cy, B x cy, B x ce) and B x REVERB_STATS
  ReverbBank bk;
  uint64_t seed, utt_offset;
  uint32_t rir_thr, noise_thr;
  int is_i16, Nmax, tiles_y, cy, ce, finish;       // finish: stage 0 of the stats kernel computes s too (no noise launch follows)
};

// S of one chunk of REVERB_POW_CHUNK elements, of which thread t holds elements t, t + 256, t + 512 and t + 768 (zero where missing): the
// halving tree v[j] += v[j + 512], + 256, ..., + 1.  The first two levels are this thread's own registers, + 128 and + 64 cross waves
// through LDS, + 32 .. + 1 are lane shifts inside wave 0.  Every thread of the workgroup calls it; thread 0 holds the result.
__device__ __forceinline__ double reverb_chunk_sum(float e0, float e1, float e2, float e3, double *red, int tid) {
  const double a0 = (double)e0 * (double)e0 + (double)e2 * (double)e2;       // a square is exact in float64: contraction changes nothing
  const double a1 = (double)e1 * (double)e1 + (double)e3 * (double)e3;
  double a = a0 + a1;
  __syncthreads();                                                           // (red may still be read by the call before)
  red[tid] = a;
  __syncthreads();
  if (tid < 128) { a = red[tid] + red[tid + 128]; red[tid] = a; }
  __syncthreads();
  if (tid < 64) {
    a = red[tid] + red[tid + 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
  }
  return a;
}

// The sum of cnt partial sums in ascending order, by one wave: 64 of them are loaded at a time and handed to the adder lane by lane.
__device__ __forceinline__ double reverb_ordered_sum(const double *p, int cnt, int lane) {
  double acc = 0.0;
  for (int base = 0; base < cnt; base += 64) {
    const double v = base + lane < cnt ? p[base + lane] : 0.0;
    const int m = min(64, cnt - base);
    for (int j = 0; j < m; ++j) acc += __shfl(v, j, 64);
  }
  return acc;
}

// One group of eight taps for the lane's eight outputs.  The window is two runs of eight samples, `lo` the newer (lower addresses) and
// `hi` the older: tap jj meets, at output r, sample m = r - jj + 7 of lo | hi.  Two groups per trip with the runs swapping roles leave
// nothing to move between trips.
template <bool TAIL>
__device__ __forceinline__ void reverb_taps8(double (&acc)[REVERB_RUN], const double (&lo)[8], const double (&hi)[8], const double *taps, int live) {
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    if (!TAIL || jj < live) {
      const double hk = taps[jj];
#pragma unroll
      for (int r = 0; r < REVERB_RUN; ++r) {
        const int m = r - jj + 7;
        acc[r] = fma(hk, m < 8 ? lo[m] : hi[m - 8], acc[r]);
      }
    }
  }
}

__device__ __forceinline__ void reverb_load8(double (&v)[8], const float *w) {
  const f32x4 a = *reinterpret_cast<const f32x4 *>(w), b = *reinterpret_cast<const f32x4 *>(w + 4);
#pragma unroll
  for (int q = 0; q < 4; ++q) { v[q] = (double)a[q]; v[4 + q] = (double)b[q]; }
}

__global__ __launch_bounds__(256) void reverb_conv_kernel(ReverbArgs a) {
  __shared__ __align__(16) double taps[REVERB_TAP_CHUNK];                    // 8 KB
  __shared__ __align__(16) float span[REVERB_TILE + REVERB_TAP_CHUNK];       // 12 KB; span[j] = x[i0 - k0 - (chunk - 1) + j]
  __shared__ double red[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const bool early = (int)blockIdx.x >= a.tiles_y;
  const int tile = early ? (int)blockIdx.x - a.tiles_y : (int)blockIdx.x;
  const int i0 = tile * REVERB_TILE;
  const size_t row = (size_t)b * a.Nmax;

  int len = n;                                                               // outputs of the signal this tile belongs to
  if (!early) {
    const int kend = min(REVERB_TILE, a.Nmax - i0);                          // elements of this tile inside the row
    const int nk = min(max(n - i0, 0), kend);
    for (int i = nk + tid; i < kend; i += 256) a.out[row + i0 + i] = 0.f;
    if (nk <= 0) return;                                                     // (the whole workgroup)
  } else if (n == 0) {
    return;
  }
  const ReverbDraw d = reverb_draw(a.bk, a.rir_thr, a.noise_thr, a.seed, a.utt_offset + (uint64_t)b);
  const float *h = nullptr;
  int K = 0;
  if (d.r >= 0) {
    const int32_t *meta = a.bk.rir_meta + 4 * d.r;
    h = a.bk.rirs + (size_t)d.r * a.bk.kstride;
    K = meta[0];
    if (early) { h += meta[2]; K = meta[3] - meta[2]; }
  }
  if (early) {
    if (d.r < 0) return;
    len = n + K - 1;
    if (i0 >= len) return;
  }

  if (K > 0) {
    double acc[REVERB_RUN];
#pragma unroll
    for (int r = 0; r < REVERB_RUN; ++r) acc[r] = 0.0;
    // taps beyond the tile's last output meet no sample
    const int nchunks = min(reverb_cdiv(K, REVERB_TAP_CHUNK), (i0 + REVERB_TILE - 1) / REVERB_TAP_CHUNK + 1);
    for (int c = 0; c < nchunks; ++c) {
      const int k0 = c * REVERB_TAP_CHUNK, kc = min(REVERB_TAP_CHUNK, K - k0);
      if (c) __syncthreads();                                                // the chunk before is read to the end
      for (int j = tid; j < REVERB_TAP_CHUNK; j += 256) taps[j] = j < kc ? (double)h[k0 + j] : 0.0;
      const int s0 = i0 - k0 - (REVERB_TAP_CHUNK - 1);
      for (int j = tid; j < REVERB_TILE + REVERB_TAP_CHUNK; j += 256) {
        const int s = s0 + j;
        span[j] = s >= 0 && s < n ? wave_sample(a.wave, a.is_i16, row + s) : 0.f;
      }
      __syncthreads();
      // output o = 8 tid + r meets tap j at span[o - j + chunk - 1]; a group of eight taps from j0 needs span[8 tid + chunk - 8 - j0 + m], m < 15
      const float *w = span + REVERB_RUN * tid + REVERB_TAP_CHUNK;
      double va[8], vb[8];
      reverb_load8(vb, w);
      int j0 = 0;
      for (; j0 + 16 <= kc; j0 += 16) {                                      // sixteen taps per trip: 128 FMAs on 16 new samples
        reverb_load8(va, w - 8 - j0);
        reverb_taps8<false>(acc, va, vb, taps + j0, 8);
        reverb_load8(vb, w - 16 - j0);
        reverb_taps8<false>(acc, vb, va, taps + j0 + 8, 8);
      }
      if (j0 < kc) {                                                         // up to fifteen taps left: a tap that does not exist adds nothing, not even 0 x
        reverb_load8(va, w - 8 - j0);
        reverb_taps8<true>(acc, va, vb, taps + j0, kc - j0);
        if (j0 + 8 < kc) {
          reverb_load8(vb, w - 16 - j0);
          reverb_taps8<true>(acc, vb, va, taps + j0 + 8, kc - j0 - 8);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < REVERB_RUN; ++r) span[REVERB_RUN * tid + r] = i0 + REVERB_RUN * tid + r < len ? (float)acc[r] : 0.f;
  } else {                                                                   // no impulse response: y = x
    for (int j = tid; j < REVERB_TILE; j += 256) span[j] = i0 + j < n ? wave_sample(a.wave, a.is_i16, row + i0 + j) : 0.f;
  }
  __syncthreads();

#pragma unroll 1
  for (int c = 0; c < REVERB_TILE / REVERB_POW_CHUNK; ++c) {
    const int base = i0 + c * REVERB_POW_CHUNK;
    if (base >= len) break;
    const int chunk = tile * (REVERB_TILE / REVERB_POW_CHUNK) + c;
    float e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = span[c * REVERB_POW_CHUNK + tid + 256 * q];
    const double sy = reverb_chunk_sum(e[0], e[1], e[2], e[3], red, tid);
    if (early) {
      if (tid == 0) a.pe[(size_t)b * a.ce + chunk] = sy;
      continue;
    }
    if (tid == 0) a.py[(size_t)b * a.cy + chunk] = sy;
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = base + tid + 256 * q;
      x[q] = 0.f;
      if (i < n) {
        a.out[row + i] = e[q];
        x[q] = wave_sample(a.wave, a.is_i16, row + i);
      }
    }
    const double sx = reverb_chunk_sum(x[0], x[1], x[2], x[3], red, tid);
    if (tid == 0) a.px[(size_t)b * a.cy + chunk] = sx;
  }
}

__global__ __launch_bounds__(64) void reverb_stats_kernel(ReverbArgs a, int stage) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  double *st = a.stats + (size_t)b * REVERB_STATS;
  if (n == 0) {
    if (lane == 0) { st[0] = st[1] = st[2] = 0.0; st[3] = 1.0; st[4] = 0.0; }
    return;
  }
  const int chunks = reverb_cdiv(n, REVERB_POW_CHUNK);
  double p_in;
  if (stage == 0) {
    const ReverbDraw d = reverb_draw(a.bk, a.rir_thr, a.noise_thr, a.seed, a.utt_offset + (uint64_t)b);
    p_in = reverb_ordered_sum(a.px + (size_t)b * a.cy, chunks, lane) / (double)n;
    double p_sig = p_in, g = 0.0;
    if (d.r >= 0) {
      const int32_t *meta = a.bk.rir_meta + 4 * d.r;
      const int ne = n + (meta[3] - meta[2]) - 1;
      p_sig = reverb_ordered_sum(a.pe + (size_t)b * a.ce, reverb_cdiv(ne, REVERB_POW_CHUNK), lane) / (double)ne;
    }
    if (d.m >= 0 && a.bk.pm[d.m] > 0.0) g = reverb_gain(a.bk.gj[d.j], p_sig, a.bk.pm[d.m]);
    if (lane == 0) { st[0] = p_in; st[1] = p_sig; st[2] = g; st[3] = 1.0; st[4] = 0.0; }
    if (!a.finish) return;
  } else {
    p_in = st[0];
  }
  const double p_out = reverb_ordered_sum((stage == 0 ? a.py : a.pz) + (size_t)b * a.cy, chunks, lane) / (double)n;
  if (lane == 0 && p_out > 0.0) { st[3] = reverb_norm(p_in, p_out); st[4] = 1.0; }
}

__global__ __launch_bounds__(256) void reverb_mix_kernel(ReverbArgs a) {
  __shared__ double red[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const int i0 = blockIdx.x * REVERB_TILE;
  if (i0 >= n) return;
  const ReverbDraw d = reverb_draw(a.bk, a.rir_thr, a.noise_thr, a.seed, a.utt_offset + (uint64_t)b);
  const bool add = d.m >= 0 && a.bk.pm[d.m] > 0.0;
  const double g = a.stats[(size_t)b * REVERB_STATS + 2];
  const float *q = add ? a.bk.noises + (size_t)d.m * a.bk.lstride : nullptr;
  const uint32_t L = add ? (uint32_t)a.bk.noise_len[d.m] : 1u;
  float *out = a.out + (size_t)b * a.Nmax;
#pragma unroll 1
  for (int c = 0; c < REVERB_TILE / REVERB_POW_CHUNK; ++c) {
    const int base = i0 + c * REVERB_POW_CHUNK;
    if (base >= n) break;
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + tid + 256 * k;
      e[k] = 0.f;
      if (i < n) {
        e[k] = out[i];
        if (add) {
          e[k] = reverb_mix(e[k], g, q[((uint32_t)d.off + (uint32_t)i) % L]);     // off < L <= 2^30 and i < 2^30: no wrap of the sum
          out[i] = e[k];
        }
      }
    }
    const double sz = reverb_chunk_sum(e[0], e[1], e[2], e[3], red, tid);
    if (tid == 0) a.pz[(size_t)b * a.cy + blockIdx.x * (REVERB_TILE / REVERB_POW_CHUNK) + c] = sz;
  }
}

__global__ __launch_bounds__(256) void reverb_scale_kernel(ReverbArgs a) {
  const int b = blockIdx.y;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const int i0 = blockIdx.x * REVERB_TILE;
  const double *st = a.stats + (size_t)b * REVERB_STATS;
  if (i0 >= n || st[4] == 0.0) return;
  const double s = st[3];
  float *out = a.out + (size_t)b * a.Nmax;
  const int end = min(i0 + REVERB_TILE, n);
  for (int i = i0 + threadIdx.x; i < end; i += 256) out[i] = reverb_scale(s, out[i]);
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------

// S(v) over n floats by the contract's shape: chunks of REVERB_POW_CHUNK, missing elements zero, the halving tree, chunk sums ascending.
static double reverb_power_sum(const float *v, long long n) {
  double acc = 0.0;
  std::vector<double> t(REVERB_POW_CHUNK);
  for (long long base = 0; base < n; base += REVERB_POW_CHUNK) {
    for (int j = 0; j < REVERB_POW_CHUNK; ++j) {
      const double e = base + j < n ? (double)v[base + j] : 0.0;
      t[j] = e * e;
    }
    for (int half = REVERB_POW_CHUNK / 2; half > 0; half >>= 1)
      for (int j = 0; j < half; ++j) t[j] += t[j + half];
    acc += t[0];
  }
  return acc;
}

// y[i] = fl32(sum_k h[k] x[i - k]), k ascending over the taps that meet a sample, for i < len.
static void reverb_convolve(const float *x, int n, const float *h, int K, float *y, long long len) {
  for (long long i = 0; i < len; ++i) {
    double acc = 0.0;
    const int k_lo = (int)std::max(0LL, i - (n - 1)), k_hi = (int)std::min((long long)K - 1, i);
    for (int k = k_lo; k <= k_hi; ++k) acc = fma((double)h[k], (double)x[i - k], acc);   // the product is exact: one rounding, as the sum's
    y[i] = (float)acc;
  }
}

}  // namespace

extern "C" int ctcn_reverb_limits(int32_t *out) {
  CTCN_REQUIRE(out, "ctcn_reverb_limits: null");
  out[0] = REVERB_TILE; out[1] = REVERB_TAP_CHUNK; out[2] = REVERB_POW_CHUNK; out[3] = REVERB_MAX_TAPS; out[4] = REVERB_MAX_SNRS; out[5] = REVERB_RUN;
  return CTCN_OK;
}

extern "C" size_t ctcn_reverb_bank_bytes(int R, int rir_stride, int N, int noise_stride, int num_snrs) {
  const char *why;
  if (reverb_shape_check(R, rir_stride, N, noise_stride, num_snrs, &why) != CTCN_OK) return 0;
  return reverb_layout(R, rir_stride, N, noise_stride).words * 4;
}

extern "C" int ctcn_reverb_bank(const float *rirs, const int32_t *rir_len, int R, int rir_stride, const float *noises, const int32_t *noise_len,
                                int N, int noise_stride, const double *snrs, int num_snrs, double sample_frequency, void *bank, size_t bank_bytes) {
  const char *why;
  const int rc = reverb_shape_check(R, rir_stride, N, noise_stride, num_snrs, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_reverb_bank: %s", why); return rc; }
  CTCN_REQUIRE((R == 0 || (rirs && rir_len)) && (N == 0 || (noises && noise_len)) && (num_snrs == 0 || snrs) && bank,
               "ctcn_reverb_bank: null argument");
  CTCN_REQUIRE(sample_frequency > 0.0 && sample_frequency <= 16777216.0, "ctcn_reverb_bank: sample_frequency %g outside (0, 2^24]", sample_frequency);
  const ReverbLayout lay = reverb_layout(R, rir_stride, N, noise_stride);
  CTCN_REQUIRE(bank_bytes >= lay.words * 4 && (reinterpret_cast<uintptr_t>(bank) & 7) == 0, "ctcn_reverb_bank: an 8-byte aligned buffer of %zu bytes needed", lay.words * 4);
  for (int r = 0; r < R; ++r) {
    CTCN_REQUIRE(rir_len[r] >= 1 && rir_len[r] <= rir_stride, "ctcn_reverb_bank: impulse response %d has %d taps (1 .. row stride %d)", r, rir_len[r], rir_stride);
    for (int k = 0; k < rir_len[r]; ++k)
      CTCN_REQUIRE(std::isfinite(rirs[(size_t)r * rir_stride + k]), "ctcn_reverb_bank: impulse response %d holds a value that is not finite", r);
  }
  for (int m = 0; m < N; ++m) {
    CTCN_REQUIRE(noise_len[m] >= 1 && noise_len[m] <= noise_stride, "ctcn_reverb_bank: noise %d has %d samples (1 .. row stride %d)", m, noise_len[m], noise_stride);
    for (int i = 0; i < noise_len[m]; ++i)
      CTCN_REQUIRE(std::isfinite(noises[(size_t)m * noise_stride + i]), "ctcn_reverb_bank: noise %d holds a value that is not finite", m);
  }
  for (int j = 0; j < num_snrs; ++j) CTCN_REQUIRE(std::isfinite(snrs[j]), "ctcn_reverb_bank: SNR %d is not finite", j);

  int32_t *w = static_cast<int32_t *>(bank);
  memset(w, 0, lay.words * 4);
  int32_t *meta = w + lay.meta, *nlen = w + lay.nlen;
  double *pm = reinterpret_cast<double *>(w + lay.dbl), *gj = pm + N;
  float *hr = reinterpret_cast<float *>(w) + lay.rirs, *qn = hr + (size_t)R * rir_stride;
  const int before = (int)floor(0.001 * sample_frequency), after = (int)floor(0.05 * sample_frequency);
  int emax = 0;
  for (int r = 0; r < R; ++r) {
    const float *src = rirs + (size_t)r * rir_stride;
    const int K = rir_len[r];
    int p = 0;
    for (int k = 1; k < K; ++k)
      if (src[k] > src[p]) p = k;                                            // the first index of the largest value
    const int lo = std::max(0, p - before), hi = std::min(K, p + after);
    CTCN_REQUIRE(hi > lo, "ctcn_reverb_bank: sample_frequency %g leaves impulse response %d an empty early window", sample_frequency, r);
    meta[4 * r] = K; meta[4 * r + 1] = p; meta[4 * r + 2] = lo; meta[4 * r + 3] = hi;
    emax = std::max(emax, hi - lo);
    memcpy(hr + (size_t)r * rir_stride, src, (size_t)K * 4);                 // behind K: zeros, whatever the caller's row holds there
  }
  for (int m = 0; m < N; ++m) {
    const float *src = noises + (size_t)m * noise_stride;
    nlen[m] = noise_len[m];
    pm[m] = reverb_power_sum(src, noise_len[m]) / (double)noise_len[m];
    memcpy(qn + (size_t)m * noise_stride, src, (size_t)noise_len[m] * 4);
  }
  for (int j = 0; j < num_snrs; ++j) gj[j] = pow(10.0, -snrs[j] / 10.0);
  w[0] = REVERB_MAGIC; w[1] = R; w[2] = N; w[3] = num_snrs; w[4] = rir_stride; w[5] = noise_stride; w[6] = emax; w[7] = 0;
  w[8] = (int32_t)lay.meta; w[9] = (int32_t)lay.nlen; w[10] = (int32_t)lay.dbl; w[11] = (int32_t)lay.rirs; w[12] = (int32_t)lay.words;
  return CTCN_OK;
}

extern "C" int ctcn_reverb_plan(const void *bank, const ctcn_reverb_opts *opts, uint64_t seed, uint64_t utt_index, int32_t *draws) {
  const char *why;
  const int rc = reverb_opts_check(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_reverb_plan: %s", why); return rc; }
  ReverbBank bk;
  CTCN_REQUIRE(draws && reverb_view(bank, bank, &bk), "ctcn_reverb_plan: null argument, or not a bank block of ctcn_reverb_bank");
  const ReverbDraw d = reverb_draw(bk, reverb_threshold(opts->rir_prob), reverb_threshold(opts->noise_prob), seed, utt_index);
  draws[0] = d.r; draws[1] = d.m; draws[2] = d.j; draws[3] = d.off;
  return CTCN_OK;
}

extern "C" size_t ctcn_reverb_ws_bytes(const void *bank_host, int B, int Nmax) {
  ReverbBank bk;
  if (!reverb_view(bank_host, bank_host, &bk) || B < 1 || B > 65535 || Nmax < 0 || Nmax > REVERB_MAX_SAMPLES) return 0;
  const size_t cy = ceil_div_z((size_t)Nmax, REVERB_POW_CHUNK), ce = ceil_div_z((size_t)Nmax + bk.emax, REVERB_POW_CHUNK);
  return (size_t)B * (3 * cy + ce + REVERB_STATS) * 8 + 8;
}

extern "C" int ctcn_reverb(const void *wave, int wave_is_int16, const int32_t *lens, const void *bank_host, const void *bank_dev,
                           const ctcn_reverb_opts *opts, uint64_t seed, uint64_t utt_offset, float *out, int B, int Nmax, void *ws,
                           size_t ws_bytes, void *stream) {
  const char *why;
  const int rc = reverb_opts_check(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_reverb: %s", why); return rc; }
  ReverbArgs a;
  CTCN_REQUIRE(reverb_view(bank_host, bank_dev, &a.bk), "ctcn_reverb: null bank, or not a bank block of ctcn_reverb_bank");
  CTCN_REQUIRE(lens && B > 0 && B <= 65535 && Nmax >= 0 && Nmax <= REVERB_MAX_SAMPLES && ((wave && out) || Nmax == 0),
               "ctcn_reverb: bad args (B %d at most 65 535, Nmax %d at most 2^30)", B, Nmax);
  CTCN_REQUIRE(wave != (const void *)out || Nmax == 0, "ctcn_reverb: out must not alias wave (the convolution gathers)");
  if (Nmax == 0) return CTCN_OK;
  const size_t need = ctcn_reverb_ws_bytes(bank_host, B, Nmax);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 7)) {
    ctcn_set_error("ctcn_reverb: an 8-byte aligned workspace of %zu bytes needed", need);
    return CTCN_EWORKSPACE;
  }
  a.wave = wave; a.lens = lens; a.out = out; a.seed = seed; a.utt_offset = utt_offset;
  a.rir_thr = reverb_threshold(opts->rir_prob); a.noise_thr = reverb_threshold(opts->noise_prob);
  a.is_i16 = wave_is_int16 != 0; a.Nmax = Nmax;
  a.tiles_y = ceil_div(Nmax, REVERB_TILE);
  a.cy = ceil_div(Nmax, REVERB_POW_CHUNK);
  a.ce = ceil_div(Nmax + a.bk.emax, REVERB_POW_CHUNK);
  a.px = static_cast<double *>(ws); a.py = a.px + (size_t)B * a.cy; a.pz = a.py + (size_t)B * a.cy; a.pe = a.pz + (size_t)B * a.cy;
  a.stats = a.pe + (size_t)B * a.ce;
  const bool any_rir = a.bk.R > 0 && a.rir_thr > 0, any_noise = a.bk.N > 0 && a.noise_thr > 0, normalize = opts->normalize != 0;
  a.finish = normalize && !any_noise;
  const int tiles_e = any_rir ? ceil_div(Nmax + a.bk.emax - 1, REVERB_TILE) : 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(reverb_conv_kernel, dim3(a.tiles_y + tiles_e, B), dim3(256), 0, s, a);
  CTCN_LAUNCH_CHECK();
  if (any_noise || normalize) {
    hipLaunchKernelGGL(reverb_stats_kernel, dim3(B), dim3(64), 0, s, a, 0);
    CTCN_LAUNCH_CHECK();
  }
  if (any_noise) {
    hipLaunchKernelGGL(reverb_mix_kernel, dim3(a.tiles_y, B), dim3(256), 0, s, a);
    CTCN_LAUNCH_CHECK();
    if (normalize) {
      hipLaunchKernelGGL(reverb_stats_kernel, dim3(B), dim3(64), 0, s, a, 1);
      CTCN_LAUNCH_CHECK();
    }
  }
  if (normalize) {
    hipLaunchKernelGGL(reverb_scale_kernel, dim3(a.tiles_y, B), dim3(256), 0, s, a);
    CTCN_LAUNCH_CHECK();
  }
  return CTCN_OK;
}

extern "C" int ctcn_reverb_host(const void *wave, int wave_is_int16, int num_samples, const void *bank, const ctcn_reverb_opts *opts, uint64_t seed,
                                uint64_t utt_index, float *out) {
  const char *why;
  const int rc = reverb_opts_check(opts, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_reverb_host: %s", why); return rc; }
  ReverbBank bk;
  CTCN_REQUIRE(reverb_view(bank, bank, &bk), "ctcn_reverb_host: null bank, or not a bank block of ctcn_reverb_bank");
  const int n = num_samples;
  CTCN_REQUIRE(n >= 0 && n <= REVERB_MAX_SAMPLES && ((wave && out) || n == 0), "ctcn_reverb_host: bad args (samples %d at most 2^30)", n);
  CTCN_REQUIRE(wave != (const void *)out || n == 0, "ctcn_reverb_host: out must not alias wave");
  if (n == 0) return CTCN_OK;
  const ReverbDraw d = reverb_draw(bk, reverb_threshold(opts->rir_prob), reverb_threshold(opts->noise_prob), seed, utt_index);
  std::vector<float> x(n);
  for (int i = 0; i < n; ++i) x[i] = wave_sample(wave, wave_is_int16 != 0, i);
  const double p_in = reverb_power_sum(x.data(), n) / (double)n;
  double p_sig = p_in;
  if (d.r >= 0) {
    const int32_t *meta = bk.rir_meta + 4 * d.r;
    const float *h = bk.rirs + (size_t)d.r * bk.kstride;
    reverb_convolve(x.data(), n, h, meta[0], out, n);
    const int E = meta[3] - meta[2];
    std::vector<float> e((size_t)n + E - 1);
    reverb_convolve(x.data(), n, h + meta[2], E, e.data(), (long long)e.size());
    p_sig = reverb_power_sum(e.data(), (long long)e.size()) / (double)e.size();
  } else {
    memcpy(out, x.data(), (size_t)n * 4);
  }
  if (d.m >= 0 && bk.pm[d.m] > 0.0) {
    const double g = reverb_gain(bk.gj[d.j], p_sig, bk.pm[d.m]);
    const float *q = bk.noises + (size_t)d.m * bk.lstride;
    const uint32_t L = (uint32_t)bk.noise_len[d.m];
    for (int i = 0; i < n; ++i) out[i] = reverb_mix(out[i], g, q[((uint32_t)d.off + (uint32_t)i) % L]);
  }
  if (opts->normalize) {
    const double p_out = reverb_power_sum(out, n) / (double)n;
    if (p_out > 0.0) {
      const double s = reverb_norm(p_in, p_out);
      for (int i = 0; i < n; ++i) out[i] = reverb_scale(s, out[i]);
    }
  }
  return CTCN_OK;
}
