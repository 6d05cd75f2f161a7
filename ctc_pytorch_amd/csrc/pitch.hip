// pitch.hip -- Kaldi's pitch features on the device: compute-kaldi-pitch-feats (NCCF over geometric lags, a Viterbi search over them, the
// probability-of-voicing correlation) and process-kaldi-pitch-feats (ctcn_pitch_frames, ctcn_pitch_plan_bytes, ctcn_pitch_plan,
// ctcn_pitch_workspace_bytes, ctcn_pitch, ctcn_pitch_process and the host twins ctcn_pitch_host, ctcn_pitch_process_host; the computation,
// step by step, and the plan layout in include/ctcn.h; the arithmetic in pitch_core.h).  The input is the batch at resample_frequency:
// ctcn_resample makes it (ops.pitch does both).
//
// pitch_var_kernel: one workgroup per utterance.  Lane i of 256 sums samples i, i + 256, ... (sum and sum of squares in float64); lane 0 adds
//   the 256 partial sums in ascending order: one fixed shape, no atomics.  Writes the utterance's ballast and its frame count.
// pitch_nccf_kernel: grid (tiles of PITCH_FT frames, utterances), 256 threads.  The tile's samples are staged once as float32 (frames overlap:
//   8 frames of 182 samples span 462), zeros behind the utterance.  One lane per frame forms the mean and e1 (a chain of W additions, eight
//   lanes busy: under a microsecond, and nothing else can start before it); then one work item per (frame, integer lag) walks the W products
//   of e2 and the inner product in sample order, and one per (frame, geometric lag) sums its taps of the two float64 rows and writes the
//   float32 planes nccf_pitch and nccf_pov (S consecutive floats per frame: coalesced).
// pitch_viterbi_kernel: one workgroup per utterance, one lane per state, a dependent chain over the frames.  Per frame a lane takes the
//   minimum of prev[j] + pen[|i - j|] over ALL j (the penalty is too weak for a band: a jump across every state costs less than one local
//   cost) with prev and the penalty table in LDS: prev[j] is one address for the whole wave (a broadcast), pen[|i - j|] consecutive doubles
//   of a mirrored copy of the table (rev[(S - 1 - i) + j]: a lane's row ascends with j, so unrolled steps read at immediate offsets, no
//   index arithmetic).  A step is four VALU instructions: the sum, v_min_f64, a compare of the new minimum with the old one and a select
//   of the index -- it moves exactly where the minimum strictly improved, so ties keep the lower j.  The j range is cut into four
//   contiguous quarters with a minimum each, so that four such chains run side by side; they are joined in ascending order with a strict
//   comparison, which is the lowest-index arg-min.  The frame's minimum is a wave reduction plus one
//   LDS word per wave: two LDS-only barriers per frame (lds_barrier: the next frame's correlation row, loaded a frame ahead, and the
//   backpointer stores stay in flight across them).  Backpointers go to global memory as 16-bit words.  The walk back stages the
//   backpointers of PITCH_RUN frames at a time in LDS with coalesced loads, one lane walks them there, and the run's output rows are then
//   written by a lane each: no dependent global load per frame.
// pitch_process_kernel: grid (tiles of 256 frames, utterances).  The tile's log pitch and voicing weights with their halo (the
//   normalisation contexts) are staged in LDS in float64; a lane per frame sums its window in ascending order, takes the delta and writes
//   the columns.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "pitch_core.h"

namespace {

constexpr int PITCH_HEADER = 16;                   // words in front of lags[]
constexpr int PITCH_MAX_STATES = 1024;
constexpr int PITCH_MAX_TAPS = 16;
constexpr int PITCH_MAX_WINDOW = 8192;             // W + last: the samples of one frame's window
constexpr int PITCH_FT = 8;                        // frames per workgroup of pitch_nccf_kernel
constexpr int PITCH_RUN = 32;                      // frames of backpointers staged at a time by the walk back
constexpr int PITCH_MAX_RATE = 1 << 24;
constexpr int PITCH_MAX_CONTEXT = 1500;            // normalisation context to either side (frames)
constexpr int PITCH_PT = 256;                      // frames per workgroup of pitch_process_kernel

struct PitchGeom {
  int fs, rf, W, shift, first, last, nm, S, taps, win;
  double c, fw, nccf_ballast, soft;
  size_t off_lags, off_pitch, off_tfirst, off_tn, off_w, off_soft, off_pen, words;
};

static inline float pitch_first_lag(const ctcn_pitch_opts *o) { return (float)(1.0 / (double)o->max_f0); }
static inline float pitch_next_lag(const ctcn_pitch_opts *o, float lag) { return (float)((double)lag * (1.0 + (double)o->delta_pitch)); }

static int pitch_geom(const ctcn_pitch_opts *o, PitchGeom *g, const char **why) {
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (!o->snip_edges) { *why = "snip_edges=false is not built"; return CTCN_EUNSUPPORTED; }
  if (o->preemphasis_coefficient != 0.f) { *why = "a preemphasis_coefficient other than 0 is not built"; return CTCN_EUNSUPPORTED; }
  if (!(o->sample_frequency > 0.f && o->resample_frequency > 0.f) || o->sample_frequency > PITCH_MAX_RATE || o->resample_frequency > PITCH_MAX_RATE ||
      o->sample_frequency != (float)(int)o->sample_frequency || o->resample_frequency != (float)(int)o->resample_frequency) {
    *why = "sample_frequency and resample_frequency must be whole numbers of Hz in (0, 2^24]"; return CTCN_EUNSUPPORTED;
  }
  if (!(o->min_f0 > 0.f && o->max_f0 > o->min_f0)) { *why = "0 < min_f0 < max_f0 needed"; return CTCN_EUNSUPPORTED; }
  if (!(o->delta_pitch > 0.f) || !(o->soft_min_f0 > 0.f) || !(o->penalty_factor >= 0.f) || !(o->nccf_ballast >= 0.f)) {
    *why = "delta_pitch and soft_min_f0 must be positive, penalty_factor and nccf_ballast not negative"; return CTCN_EUNSUPPORTED;
  }
  if (o->lowpass_filter_width <= 0 || o->upsample_filter_width <= 0) { *why = "filter widths must be positive"; return CTCN_EUNSUPPORTED; }
  g->fs = (int)o->sample_frequency; g->rf = (int)o->resample_frequency;
  if (!(o->lowpass_cutoff > 0.f) || (double)o->lowpass_cutoff * 2 > std::min(g->fs, g->rf)) {
    *why = "lowpass_cutoff must be positive and at most the Nyquist frequency of the lower rate"; return CTCN_EUNSUPPORTED;
  }
  const double rf = g->rf;
  const double w = rf * (double)o->frame_length / 1000.0, sh = rf * (double)o->frame_shift / 1000.0;
  if (!(w >= 1.0 && sh >= 1.0 && w <= PITCH_MAX_WINDOW && sh <= PITCH_MAX_WINDOW)) { *why = "frame_length or frame_shift outside the kernel's range"; return CTCN_EUNSUPPORTED; }
  g->W = (int)w; g->shift = (int)sh;
  const double half = (double)o->upsample_filter_width / (2.0 * rf);
  const double lo = ceil(rf * (1.0 / (double)o->max_f0 - half)), hi = floor(rf * (1.0 / (double)o->min_f0 + half));
  if (!(lo >= 0.0 && hi >= lo && hi + g->W <= PITCH_MAX_WINDOW)) { *why = "measured lags outside the kernel's range (W + last lag at most 8192 samples)"; return CTCN_EUNSUPPORTED; }
  g->first = (int)lo; g->last = (int)hi; g->nm = g->last - g->first + 1; g->win = g->W + g->last;
  int S = 0;
  const float max_lag = (float)(1.0 / (double)o->min_f0);
  for (float lag = pitch_first_lag(o); lag <= max_lag; lag = pitch_next_lag(o, lag)) {
    float next = pitch_next_lag(o, lag);
    if (++S > PITCH_MAX_STATES || !(next > lag)) { *why = "more than 1024 lags (states of the Viterbi search)"; return CTCN_EUNSUPPORTED; }
  }
  if (S < 1) { *why = "no lags"; return CTCN_EUNSUPPORTED; }
  g->S = S;
  g->fw = (double)o->upsample_filter_width / (2.0 * (rf / 2.0));   // num_zeros / (2 cutoff), cutoff = rf / 2
  int taps = 0;
  {
    float lag = pitch_first_lag(o);
    for (int i = 0; i < S; ++i, lag = pitch_next_lag(o, lag)) {
      const double t = (double)lag - (double)g->first / rf;
      const int a = std::max((int)ceil(rf * (t - g->fw)), 0), b = std::min((int)floor(rf * (t + g->fw)), g->nm - 1);
      if (b < a) { *why = "a lag without taps"; return CTCN_EUNSUPPORTED; }
      taps = std::max(taps, b - a + 1);
    }
  }
  if (taps > PITCH_MAX_TAPS) { *why = "more than 16 upsampling taps per lag"; return CTCN_EUNSUPPORTED; }
  g->taps = taps;
  const double lg = log(1.0 + (double)o->delta_pitch);
  g->c = (lg * lg) * (double)o->penalty_factor;
  g->nccf_ballast = (double)o->nccf_ballast;
  g->soft = (double)o->soft_min_f0;
  size_t p = PITCH_HEADER;
  g->off_lags = p; p += S;
  g->off_pitch = p; p += S;
  g->off_tfirst = p; p += S;
  g->off_tn = p; p += S;
  g->off_w = p; p += (size_t)S * taps;
  p += p & 1;                                                         // doubles on 8-byte boundaries
  g->off_soft = p; p += 2 * (size_t)S;
  g->off_pen = p; p += 2 * (size_t)S;
  g->words = p;
  return CTCN_OK;
}

static inline long long pitch_downsampled(long long n, const PitchGeom &g) { return n <= 0 ? 0 : (n * g.rf + g.fs - 1) / g.fs; }
__host__ __device__ inline int pitch_frame_count(int m, int W, int shift) { return m < W ? 0 : (m - W) / shift + 1; }

struct PitchPlanView {
  const float *lags, *pitch, *w;
  const int32_t *tfirst, *tn;
  const double *soft, *pen;
};

static inline PitchPlanView pitch_view(const void *plan, const PitchGeom &g) {
  const int32_t *p = static_cast<const int32_t *>(plan);
  PitchPlanView v;
  v.lags = reinterpret_cast<const float *>(p + g.off_lags);
  v.pitch = reinterpret_cast<const float *>(p + g.off_pitch);
  v.tfirst = p + g.off_tfirst;
  v.tn = p + g.off_tn;
  v.w = reinterpret_cast<const float *>(p + g.off_w);
  v.soft = reinterpret_cast<const double *>(p + g.off_soft);
  v.pen = reinterpret_cast<const double *>(p + g.off_pen);
  return v;
}

struct PitchWs {
  double *ballast;
  float *nccf_pitch, *nccf_pov;
  unsigned short *bp;
  size_t bytes;
};

static inline PitchWs pitch_ws(void *ws, int B, int Tmax, int S) {
  char *p = static_cast<char *>(ws);
  const size_t cells = (size_t)B * Tmax * S;
  PitchWs w;
  size_t off = 0;
  w.ballast = reinterpret_cast<double *>(p + off); off += align_up((size_t)B * 8, 256);
  w.nccf_pitch = reinterpret_cast<float *>(p + off); off += align_up(cells * 4, 256);
  w.nccf_pov = reinterpret_cast<float *>(p + off); off += align_up(cells * 4, 256);
  w.bp = reinterpret_cast<unsigned short *>(p + off); off += align_up(cells * 2, 256);
  w.bytes = off;
  return w;
}

struct PitchArgs {
  const float *wave;
  const int32_t *lens;
  PitchPlanView plan;
  PitchWs ws;
  float *out;
  int32_t *lag_index, *frames;
  int Mmax, Tmax, W, shift, first, nm, S, taps, win;
  double nccf_ballast;
};

__global__ __launch_bounds__(PITCH_VAR_LANES) void pitch_var_kernel(PitchArgs a) {
  __shared__ double s[PITCH_VAR_LANES], q[PITCH_VAR_LANES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int m = min(max(a.lens[b], 0), a.Mmax);
  const float *x = a.wave + (size_t)b * a.Mmax;
  double S = 0.0, Q = 0.0;
  for (int k = tid; k < m; k += PITCH_VAR_LANES) pitch_var_add(&S, &Q, x[k]);
  s[tid] = S;
  q[tid] = Q;
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0, tq = 0.0;
    for (int i = 0; i < PITCH_VAR_LANES; ++i) {
      ts = ts + s[i];
      tq = tq + q[i];
    }
    a.ws.ballast[b] = m > 0 ? pitch_ballast(ts, tq, m, a.W, a.nccf_ballast) : 0.0;
    a.frames[b] = min(pitch_frame_count(m, a.W, a.shift), a.Tmax);
  }
}

__global__ __launch_bounds__(256) void pitch_nccf_kernel(PitchArgs a) {
  extern __shared__ __align__(16) double smem_pd[];
  const int nm = a.nm, S = a.S, W = a.W, shift = a.shift;
  double *nc = smem_pd;                                               // PITCH_FT x nm x 2: nccf_pitch, nccf_pov of the integer lags
  double *mean = nc + PITCH_FT * nm * 2, *e1 = mean + PITCH_FT;
  float *xs = reinterpret_cast<float *>(e1 + PITCH_FT);               // (PITCH_FT - 1) shift + W + last samples
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m = min(max(a.lens[b], 0), a.Mmax);
  const int T = min(pitch_frame_count(m, W, shift), a.Tmax);
  const int t0 = blockIdx.x * PITCH_FT;
  const int nf = min(PITCH_FT, T - t0);
  if (nf <= 0) return;                                                // (the whole workgroup)
  const float *x = a.wave + (size_t)b * a.Mmax;
  const int span = (nf - 1) * shift + a.win;
  const long long s0 = (long long)t0 * shift;
  for (int i = tid; i < span; i += 256) xs[i] = s0 + i < m ? x[s0 + i] : 0.f;
  __syncthreads();
  if (tid < nf) pitch_frame_mean(xs + tid * shift, W, &mean[tid], &e1[tid]);
  __syncthreads();
  const double ballast = a.ws.ballast[b];
  for (int item = tid; item < nf * nm; item += 256) {
    const int f = item / nm, l = item - f * nm;
    pitch_nccf_lag(xs + f * shift, W, a.first + l, mean[f], e1[f], ballast, &nc[item * 2], &nc[item * 2 + 1]);
  }
  __syncthreads();
  for (int item = tid; item < nf * S; item += 256) {
    const int f = item / S, i = item - f * S;
    const double *row = nc + ((size_t)f * nm + a.plan.tfirst[i]) * 2;
    const float *w = a.plan.w + (size_t)i * a.taps;
    const int n = a.plan.tn[i];
    const size_t o = ((size_t)b * a.Tmax + t0 + f) * S + i;
    a.ws.nccf_pitch[o] = pitch_upsample(row, 2, w, n);
    a.ws.nccf_pov[o] = pitch_upsample(row + 1, 2, w, n);
  }
}

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(1024) void pitch_viterbi_kernel(PitchArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) double smem_pd[];
  const int S = a.S, SP = blockDim.x;                                 // SP: S rounded up to whole waves
  double *prev = smem_pd;                                             // 2 x SP
  double *rev = prev + 2 * SP;                                        // 2 SP: rev[k] = pen[|k - (S - 1)|], so that pen[|i - j|] = rev[(S - 1 - i) + j]
  double *wmin = rev + 2 * SP;                                        // 16
  int *path = reinterpret_cast<int *>(wmin + 16);                     // PITCH_RUN
  unsigned short *bps = reinterpret_cast<unsigned short *>(path + PITCH_RUN);   // PITCH_RUN x S
  const int b = blockIdx.x, i = threadIdx.x, nw = SP >> 6;
  const bool active = i < S;
  const int m = min(max(a.lens[b], 0), a.Mmax);
  const int T = min(pitch_frame_count(m, a.W, a.shift), a.Tmax);
  const size_t row0 = (size_t)b * a.Tmax;
  for (int k = i; k < (a.Tmax - T) * 2; k += SP) a.out[(row0 + T) * 2 + k] = 0.f;
  if (a.lag_index)
    for (int k = i; k < a.Tmax - T; k += SP) a.lag_index[row0 + T + k] = 0;
  if (T <= 0) return;                                                 // (the whole workgroup)
  for (int k = i; k < 2 * S - 1; k += SP) rev[k] = a.plan.pen[abs(k - (S - 1))];
  const double *pr = rev + (active ? S - 1 - i : 0);                  // this lane's row of penalties, ascending in j
  prev[i] = 0.0;
  const double soft = active ? a.plan.soft[i] : 0.0;
  const float *np = a.ws.nccf_pitch + row0 * S + (active ? i : 0);
  unsigned short *bp = a.ws.bp + row0 * S + (active ? i : 0);
  float nxt = np[0];
  const double inf = __builtin_huge_val();
  const int q = (S + 3) >> 2;
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    const float n = nxt;
    if (t + 1 < T) nxt = np[(size_t)(t + 1) * S];
    const double *pv = prev + cur * SP;
    double fwd = inf;
    int arg = 0;
    if (active) {
      // A step of one chain: the minimum by v_min_f64, and the index moves exactly where the minimum did (a strict improvement: ties keep
      // the lower j).  Candidates are sums of two values that are never -0.0, so the minimum of equal values is either of them.
      double b0 = inf, b1 = inf, b2 = inf, b3 = inf;
      int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#define PITCH_STEP(B_, A_, J_)                    \
  {                                               \
    const double c_ = pv[J_] + pr[J_];            \
    const double m_ = fmin(B_, c_);               \
    A_ = m_ != B_ ? (J_) : A_;                    \
    B_ = m_;                                      \
  }
      const int n3 = S - 3 * q;                                        // the last quarter's length (at most q; below 1 only where S < 4)
      const int common = n3 > 0 ? n3 : 0;
      int jj = 0;
#pragma unroll 4
      for (; jj < common; ++jj) {                                      // all four quarters: no bound to test
        PITCH_STEP(b0, a0, jj)
        PITCH_STEP(b1, a1, q + jj)
        PITCH_STEP(b2, a2, 2 * q + jj)
        PITCH_STEP(b3, a3, 3 * q + jj)
      }
      for (; jj < q; ++jj) {                                           // at most three rounds, or S < 4
        PITCH_STEP(b0, a0, jj)
        if (q + jj < S) PITCH_STEP(b1, a1, q + jj)
        if (2 * q + jj < S) PITCH_STEP(b2, a2, 2 * q + jj)
      }
#undef PITCH_STEP
      double best = b0;
      arg = a0;
      if (b1 < best) { best = b1; arg = a1; }
      if (b2 < best) { best = b2; arg = a2; }
      if (b3 < best) { best = b3; arg = a3; }
      fwd = pitch_local(n, soft) + best;
    }
    const double wm = wave_min_d(fwd);
    if ((i & 63) == 0) wmin[i >> 6] = wm;
    lds_barrier();
    double mn = wmin[0];
    for (int w = 1; w < nw; ++w) mn = fmin(mn, wmin[w]);
    if (active) {
      prev[(cur ^ 1) * SP + i] = fwd - mn;
      bp[(size_t)t * S] = (unsigned short)arg;
    }
    lds_barrier();
    cur ^= 1;
  }
  __syncthreads();                                                    // every backpointer store has landed
  int state = 0;
  if (i == 0) {
    const double *pv = prev + cur * SP;
    double best = pv[0];
    for (int j = 1; j < S; ++j)
      if (pv[j] < best) { best = pv[j]; state = j; }
  }
  for (int r = (T - 1) / PITCH_RUN; r >= 0; --r) {
    const int tlo = r * PITCH_RUN, cnt = min(T - tlo, PITCH_RUN);
    const unsigned short *src = a.ws.bp + (row0 + tlo) * S;
    for (int k = i; k < cnt * S; k += SP) bps[k] = src[k];
    __syncthreads();
    if (i == 0) {
      for (int k = cnt - 1; k >= 0; --k) {
        path[k] = state;
        if (tlo + k > 0) state = bps[k * S + state];
      }
    }
    __syncthreads();
    if (i < cnt) {
      const int st = path[i];
      const size_t t = row0 + tlo + i;
      a.out[t * 2] = a.ws.nccf_pov[t * S + st];
      a.out[t * 2 + 1] = a.plan.pitch[st];
      if (a.lag_index) a.lag_index[t] = st;
    }
    __syncthreads();
  }
}

// N(0, 1) of frame `frame` of utterance `utt`: fbank.hip's keying with sample 0 (Box-Muller's cosine), float32 on both sides
__host__ __device__ inline float pitch_gauss(uint64_t seed, uint64_t utt, int frame) {
  uint32_t w[4];
  philox4(seed, (utt << 38) | ((uint64_t)(uint32_t)frame << 10), w);
  const float u1 = ((float)(w[0] >> 8) + 1.0f) * 5.9604644775390625e-08f;      // (0, 1]
  const float th = 6.28318530717958647692f * ((float)(w[1] >> 8) * 5.9604644775390625e-08f);
  return sqrtf(-2.0f * logf(u1)) * cosf(th);
}

struct ProcessGeom {
  int left, right, dw, cols, halo_l, halo_r;
  float scales[16];
};

static int process_geom(const ctcn_pitch_process_opts *o, ProcessGeom *g, const char **why) {
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (o->delay != 0) { *why = "a delay other than 0 is not built"; return CTCN_EUNSUPPORTED; }
  if (o->normalization_left_context < 0 || o->normalization_right_context < 0 || o->normalization_left_context > PITCH_MAX_CONTEXT ||
      o->normalization_right_context > PITCH_MAX_CONTEXT) { *why = "normalisation contexts outside [0, 1500]"; return CTCN_EUNSUPPORTED; }
  if (o->delta_window < 1 || o->delta_window > 5) { *why = "delta_window outside [1, 5]"; return CTCN_EUNSUPPORTED; }
  if (!(o->delta_pitch_noise_stddev >= 0.f)) { *why = "delta_pitch_noise_stddev must not be negative"; return CTCN_EINVAL; }
  g->cols = (o->add_pov_feature != 0) + (o->add_normalized_log_pitch != 0) + (o->add_delta_pitch != 0) + (o->add_raw_log_pitch != 0);
  if (g->cols == 0) { *why = "no column asked for"; return CTCN_EINVAL; }
  g->left = o->normalization_left_context; g->right = o->normalization_right_context; g->dw = o->delta_window;
  g->halo_l = std::max(g->left, g->dw); g->halo_r = std::max(g->right, g->dw);
  if (ctcn_delta_scales(1, g->dw, g->scales) != 2 * g->dw + 1) { *why = "no delta scales"; return CTCN_EUNSUPPORTED; }
  return CTCN_OK;
}

struct ProcessArgs {
  const float *raw;
  const int32_t *frames;
  float *out;
  int Tmax, left, right, dw, cols, halo_l, halo_r, add_pov, add_norm, add_delta, add_raw;
  float pitch_scale, pov_scale, pov_offset, delta_scale, stddev;
  float scales[16];
  uint64_t seed, utt_offset;
};

// The columns of frame t of an utterance of T frames; lp / pw hold log pitch and voicing weight of frame u at index u - base.
__host__ __device__ inline void pitch_process_frame(const ProcessArgs &a, const double *lp, const double *pw, int base, int t, int T, float nccf,
                                                    uint64_t utt, float *o) {
#pragma clang fp contract(off)
  int c = 0;
  if (a.add_pov) o[c++] = (float)((double)a.pov_scale * pitch_pov_feature((double)nccf) + (double)a.pov_offset);
  if (a.add_norm) {
    const int u0 = t - a.left > 0 ? t - a.left : 0, u1 = t + a.right < T - 1 ? t + a.right : T - 1;
    double s0 = 0.0, s1 = 0.0;
    for (int u = u0; u <= u1; ++u) {
      const double p = pw[u - base];
      s0 = s0 + p;
      s1 = s1 + p * lp[u - base];
    }
    o[c++] = (float)((double)a.pitch_scale * (lp[t - base] - s1 / s0));
  }
  if (a.add_delta) {
    double d = 0.0;
    for (int k = -a.dw; k <= a.dw; ++k) {
      int u = t + k;
      u = u < 0 ? 0 : (u > T - 1 ? T - 1 : u);
      d = d + (double)a.scales[k + a.dw] * lp[u - base];
    }
    if (a.stddev > 0.f) d = d + (double)a.stddev * (double)pitch_gauss(a.seed, utt, t);
    o[c++] = (float)((double)a.delta_scale * d);
  }
  if (a.add_raw) o[c++] = (float)lp[t - base];
}

__global__ __launch_bounds__(PITCH_PT) void pitch_process_kernel(ProcessArgs a) {
  extern __shared__ __align__(16) double smem_pd[];
  const int len = PITCH_PT + a.halo_l + a.halo_r;
  double *lp = smem_pd, *pw = lp + len;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int T = min(max(a.frames[b], 0), a.Tmax);
  const int t0 = blockIdx.x * PITCH_PT, t = t0 + tid;
  const size_t row0 = (size_t)b * a.Tmax;
  if (t0 < T) {                                                       // (the whole workgroup)
    const int base = t0 - a.halo_l;
    for (int k = tid; k < len; k += PITCH_PT) {
      const int u = base + k;
      if (u >= 0 && u < T) {
        lp[k] = log((double)a.raw[(row0 + u) * 2 + 1]);
        pw[k] = pitch_pov((double)a.raw[(row0 + u) * 2]);
      }
    }
    __syncthreads();
    if (t < T) {
      float o[4];
      pitch_process_frame(a, lp, pw, base, t, T, a.raw[(row0 + t) * 2], (uint64_t)b + a.utt_offset, o);
      for (int c = 0; c < a.cols; ++c) a.out[(row0 + t) * a.cols + c] = o[c];
    }
  }
  if (t >= T && t < a.Tmax)
    for (int c = 0; c < a.cols; ++c) a.out[(row0 + t) * a.cols + c] = 0.f;
}

static void process_args(const ctcn_pitch_process_opts *o, const ProcessGeom &g, ProcessArgs *a) {
  a->left = g.left; a->right = g.right; a->dw = g.dw; a->cols = g.cols; a->halo_l = g.halo_l; a->halo_r = g.halo_r;
  a->add_pov = o->add_pov_feature != 0; a->add_norm = o->add_normalized_log_pitch != 0; a->add_delta = o->add_delta_pitch != 0;
  a->add_raw = o->add_raw_log_pitch != 0;
  a->pitch_scale = o->pitch_scale; a->pov_scale = o->pov_scale; a->pov_offset = o->pov_offset; a->delta_scale = o->delta_pitch_scale;
  a->stddev = o->delta_pitch_noise_stddev;
  memcpy(a->scales, g.scales, sizeof(a->scales));
}

}  // namespace

extern "C" int ctcn_pitch_frames(long long num_samples, const ctcn_pitch_opts *opts) {
  PitchGeom g;
  const char *why;
  const int rc = pitch_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_pitch_frames: %s", why); return rc; }
  CTCN_REQUIRE(num_samples >= 0 && num_samples < (1LL << 38), "ctcn_pitch_frames: bad sample count %lld", num_samples);
  const long long m = pitch_downsampled(num_samples, g);
  if (m > 0x7fffffffLL) { ctcn_set_error("ctcn_pitch_frames: %lld downsampled samples, beyond int", m); return CTCN_EUNSUPPORTED; }
  return pitch_frame_count((int)m, g.W, g.shift);
}

extern "C" size_t ctcn_pitch_plan_bytes(const ctcn_pitch_opts *opts) {
  PitchGeom g;
  const char *why;
  return pitch_geom(opts, &g, &why) == CTCN_OK ? g.words * 4 : 0;
}

extern "C" int ctcn_pitch_plan(const ctcn_pitch_opts *opts, void *plan, size_t plan_bytes) {
  PitchGeom g;
  const char *why;
  const int rc = pitch_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_pitch_plan: %s", why); return rc; }
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4 && ((uintptr_t)plan & 7) == 0, "ctcn_pitch_plan: an 8-byte aligned buffer of %zu bytes needed", g.words * 4);
  memset(plan, 0, g.words * 4);
  int32_t *hdr = static_cast<int32_t *>(plan);
  hdr[0] = g.S; hdr[1] = g.first; hdr[2] = g.last; hdr[3] = g.W; hdr[4] = g.shift; hdr[5] = g.taps; hdr[6] = PITCH_RUN; hdr[7] = g.nm;
  float *lags = reinterpret_cast<float *>(hdr + g.off_lags), *pitch = reinterpret_cast<float *>(hdr + g.off_pitch);
  int32_t *tfirst = hdr + g.off_tfirst, *tn = hdr + g.off_tn;
  float *wts = reinterpret_cast<float *>(hdr + g.off_w);
  double *soft = reinterpret_cast<double *>(hdr + g.off_soft), *pen = reinterpret_cast<double *>(hdr + g.off_pen);
  const double two_pi = 6.283185307179586476925286766559, pi = 3.14159265358979323846264338327950288;
  const double rf = g.rf, cutoff = rf / 2.0;
  const int nz = opts->upsample_filter_width;
  float lag = pitch_first_lag(opts);
  for (int i = 0; i < g.S; ++i, lag = pitch_next_lag(opts, lag)) {
    lags[i] = lag;
    pitch[i] = 1.0f / lag;
    soft[i] = g.soft * (double)lag;
    pen[i] = (double)((long long)i * i) * g.c;
    const double t = (double)lag - (double)g.first / rf;
    const int a = std::max((int)ceil(rf * (t - g.fw)), 0), b = std::min((int)floor(rf * (t + g.fw)), g.nm - 1);
    tfirst[i] = a;
    tn[i] = b - a + 1;
    for (int j = a; j <= b; ++j) {
      const double d = t - (double)j / rf;
      const double win = fabs(d) < g.fw ? 0.5 * (1 + cos(two_pi * cutoff / nz * d)) : 0.0;
      const double filt = d != 0.0 ? sin(two_pi * cutoff * d) / (pi * d) : 2 * cutoff;
      wts[(size_t)i * g.taps + (j - a)] = (float)(filt * win / rf);
    }
  }
  return CTCN_OK;
}

extern "C" size_t ctcn_pitch_workspace_bytes(const ctcn_pitch_opts *opts, int B, int Tmax) {
  PitchGeom g;
  const char *why;
  if (pitch_geom(opts, &g, &why) != CTCN_OK || B <= 0 || Tmax < 0) return 0;
  return pitch_ws(nullptr, B, Tmax, g.S).bytes;
}

extern "C" int ctcn_pitch(const float *wave, const int32_t *lens, const ctcn_pitch_opts *opts, const void *plan, float *out, int32_t *lag_index,
                          int32_t *frames, int B, int Mmax, int Tmax, void *ws, size_t ws_bytes, void *stream) {
  PitchGeom g;
  const char *why;
  const int rc = pitch_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_pitch: %s", why); return rc; }
  CTCN_REQUIRE(lens && plan && frames && ws && B > 0 && B <= 65535 && Mmax >= 0 && Tmax >= 0 && (wave || Mmax == 0) && (out || Tmax == 0),
               "ctcn_pitch: bad args (B %d at most 65 535)", B);
  CTCN_REQUIRE(((uintptr_t)plan & 7) == 0 && ((uintptr_t)ws & 255) == 0, "ctcn_pitch: plan must be 8-byte, workspace 256-byte aligned");
  CTCN_REQUIRE(Tmax <= pitch_frame_count(Mmax, g.W, g.shift), "ctcn_pitch: Tmax %d beyond the %d frames %d samples hold", Tmax,
               pitch_frame_count(Mmax, g.W, g.shift), Mmax);
  CTCN_REQUIRE((size_t)B * Tmax <= (size_t)0x7fffffff / g.S, "ctcn_pitch: B x Tmax x S beyond 2^31");
  PitchArgs a;
  a.ws = pitch_ws(ws, B, Tmax, g.S);
  if (ws_bytes < a.ws.bytes) { ctcn_set_error("ctcn_pitch: workspace of %zu bytes needed, %zu given", a.ws.bytes, ws_bytes); return CTCN_EWORKSPACE; }
  a.wave = wave; a.lens = lens; a.plan = pitch_view(plan, g); a.out = out; a.lag_index = lag_index; a.frames = frames;
  a.Mmax = Mmax; a.Tmax = Tmax; a.W = g.W; a.shift = g.shift; a.first = g.first; a.nm = g.nm; a.S = g.S; a.taps = g.taps; a.win = g.win;
  a.nccf_ballast = g.nccf_ballast;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pitch_var_kernel, dim3(B), dim3(PITCH_VAR_LANES), 0, st, a);
  CTCN_LAUNCH_CHECK();
  if (Tmax == 0) return CTCN_OK;
  const size_t lds_n = ((size_t)PITCH_FT * g.nm * 2 + 2 * PITCH_FT) * 8 + ((size_t)(PITCH_FT - 1) * g.shift + g.win) * 4;
  if (lds_n > 160 * 1024) { ctcn_set_error("ctcn_pitch: a tile of %zu bytes, beyond the LDS", lds_n); return CTCN_EUNSUPPORTED; }
  if (lds_n > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pitch_nccf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_n));
  hipLaunchKernelGGL(pitch_nccf_kernel, dim3(ceil_div(Tmax, PITCH_FT), B), dim3(256), lds_n, st, a);
  CTCN_LAUNCH_CHECK();
  const int SP = ceil_div(g.S, 64) * 64;
  const size_t lds_v = ((size_t)4 * SP + 16) * 8 + PITCH_RUN * 4 + (size_t)PITCH_RUN * g.S * 2;
  if (lds_v > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pitch_viterbi_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_v));
  hipLaunchKernelGGL(pitch_viterbi_kernel, dim3(B), dim3(SP), lds_v, st, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_pitch_host(const float *wave, int num_samples, const ctcn_pitch_opts *opts, const void *plan, float *out, int32_t *lag_index,
                               int out_cap) {
#pragma clang fp contract(off)
  PitchGeom g;
  const char *why;
  const int rc = pitch_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_pitch_host: %s", why); return rc; }
  CTCN_REQUIRE(plan && ((uintptr_t)plan & 7) == 0 && num_samples >= 0 && out_cap >= 0 && (wave || num_samples == 0) && (out || out_cap == 0),
               "ctcn_pitch_host: bad args");
  const int32_t *hdr = static_cast<const int32_t *>(plan);
  CTCN_REQUIRE(hdr[0] == g.S && hdr[1] == g.first && hdr[2] == g.last && hdr[3] == g.W && hdr[4] == g.shift && hdr[5] == g.taps,
               "ctcn_pitch_host: the plan is not the one of these options");
  const PitchPlanView pv = pitch_view(plan, g);
  const int m = num_samples, S = g.S, T = pitch_frame_count(m, g.W, g.shift);
  CTCN_REQUIRE(T <= out_cap, "ctcn_pitch_host: %d frames, room for %d", T, out_cap);
  if (T == 0) return 0;
  double ps[PITCH_VAR_LANES], pq[PITCH_VAR_LANES];
  for (int i = 0; i < PITCH_VAR_LANES; ++i) {
    double s = 0.0, q = 0.0;
    for (int k = i; k < m; k += PITCH_VAR_LANES) pitch_var_add(&s, &q, wave[k]);
    ps[i] = s; pq[i] = q;
  }
  double ts = 0.0, tq = 0.0;
  for (int i = 0; i < PITCH_VAR_LANES; ++i) { ts = ts + ps[i]; tq = tq + pq[i]; }
  const double ballast = pitch_ballast(ts, tq, m, g.W, g.nccf_ballast);
  std::vector<float> xs(g.win), pov((size_t)T * S);
  std::vector<double> nc((size_t)g.nm * 2), prev(S, 0.0), fwd(S);
  std::vector<unsigned short> bp((size_t)T * S);
  for (int t = 0; t < T; ++t) {
    const long long s0 = (long long)t * g.shift;
    for (int i = 0; i < g.win; ++i) xs[i] = s0 + i < m ? wave[s0 + i] : 0.f;
    double mean, e1;
    pitch_frame_mean(xs.data(), g.W, &mean, &e1);
    for (int l = 0; l < g.nm; ++l) pitch_nccf_lag(xs.data(), g.W, g.first + l, mean, e1, ballast, &nc[2 * l], &nc[2 * l + 1]);
    double mn = 0.0;
    for (int i = 0; i < S; ++i) {
      const double *row = nc.data() + (size_t)pv.tfirst[i] * 2;
      const float *w = pv.w + (size_t)i * g.taps;
      const float np = pitch_upsample(row, 2, w, pv.tn[i]);
      pov[(size_t)t * S + i] = pitch_upsample(row + 1, 2, w, pv.tn[i]);
      double best = prev[0] + pv.pen[i];
      int arg = 0;
      for (int j = 1; j < S; ++j) {
        const double c = prev[j] + pv.pen[abs(i - j)];
        if (c < best) { best = c; arg = j; }
      }
      fwd[i] = pitch_local(np, pv.soft[i]) + best;
      bp[(size_t)t * S + i] = (unsigned short)arg;
      if (i == 0 || fwd[i] < mn) mn = fwd[i];
    }
    for (int i = 0; i < S; ++i) prev[i] = fwd[i] - mn;
  }
  int state = 0;
  for (int j = 1; j < S; ++j)
    if (prev[j] < prev[state]) state = j;
  for (int t = T - 1; t >= 0; --t) {
    out[(size_t)t * 2] = pov[(size_t)t * S + state];
    out[(size_t)t * 2 + 1] = pv.pitch[state];
    if (lag_index) lag_index[t] = state;
    if (t > 0) state = bp[(size_t)t * S + state];
  }
  return T;
}

extern "C" int ctcn_pitch_process(const float *raw, const int32_t *frames, const ctcn_pitch_process_opts *opts, float *out, int B, int Tmax,
                                  uint64_t seed, uint64_t utt_offset, void *stream) {
  ProcessGeom g;
  const char *why;
  const int rc = process_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_pitch_process: %s", why); return rc; }
  CTCN_REQUIRE(raw && frames && out && B > 0 && B <= 65535 && Tmax > 0 && Tmax <= (1 << 30), "ctcn_pitch_process: bad args (B %d at most 65 535, Tmax %d)", B, Tmax);
  const uintptr_t r0 = (uintptr_t)raw, o0 = (uintptr_t)out;
  CTCN_REQUIRE(r0 + (size_t)B * Tmax * 8 <= o0 || o0 + (size_t)B * Tmax * g.cols * 4 <= r0, "ctcn_pitch_process: out must not overlap raw");
  ProcessArgs a;
  process_args(opts, g, &a);
  a.raw = raw; a.frames = frames; a.out = out; a.Tmax = Tmax; a.seed = seed; a.utt_offset = utt_offset;
  const size_t lds = (size_t)(PITCH_PT + g.halo_l + g.halo_r) * 16;
  hipLaunchKernelGGL(pitch_process_kernel, dim3(ceil_div(Tmax, PITCH_PT), B), dim3(PITCH_PT), lds, (hipStream_t)stream, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_pitch_process_host(const float *raw, int num_frames, const ctcn_pitch_process_opts *opts, uint64_t seed, uint64_t utt_index,
                                       float *out) {
  ProcessGeom g;
  const char *why;
  const int rc = process_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_pitch_process_host: %s", why); return rc; }
  const int T = num_frames;
  CTCN_REQUIRE(T >= 0 && T <= (1 << 30) && ((raw && out) || T == 0), "ctcn_pitch_process_host: bad args (frames %d)", T);
  ProcessArgs a;
  process_args(opts, g, &a);
  a.raw = raw; a.frames = nullptr; a.out = out; a.Tmax = T; a.seed = seed; a.utt_offset = 0;
  std::vector<double> lp(T), pw(T);
  for (int t = 0; t < T; ++t) {
    lp[t] = log((double)raw[(size_t)t * 2 + 1]);
    pw[t] = pitch_pov((double)raw[(size_t)t * 2]);
  }
  for (int t = 0; t < T; ++t) pitch_process_frame(a, lp.data(), pw.data(), 0, t, T, raw[(size_t)t * 2], utt_index, out + (size_t)t * g.cols);
  return g.cols;
}
