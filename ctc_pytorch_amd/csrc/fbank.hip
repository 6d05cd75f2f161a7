// fbank.hip -- the spectral front-ends: waveform -> (normalised) log-mel features (ctcn_fbank_frames, ctcn_fbank_plan, ctcn_fbank), MFCCs
// (ctcn_mfcc_plan, ctcn_mfcc) and Kaldi's spectrogram (ctcn_spectrogram) by one kernel, the recipe's log-magnitude STFT with its
// per-utterance normalisation (ctcn_logspec: logspec_kernel / logspec_finish_kernel), and ctcn_fbank_power_host, the transform on the host.
// Contract and plan layouts in include/ctcn.h; the statistics of the global normalisation are cmvn.hip's.
//
// fbank_kernel<NPAD, KIND>: grid (frame blocks, utterances), four waves per workgroup; the prologue (frame_block_begin), the transform (wave_rfft)
//   and the form of the LDS layout (a struct in fbank_core.h: the kernel reads through it, the launch sizes from it) are shared with logspec_kernel.
//   1. The workgroup stages the plan (float64 twiddles, window, filter table, weights: 6 NPAD + 384 words) and the sample span of its `fpw` (<= 8)
//      consecutive frames in LDS once: neighbouring frames share all but `shift` of their samples.  int16 input is converted here;
//      snip_edges == 0 reflects indices outside the signal here.
//   2. One wave owns one frame at a time, lane l holding samples l, l + 64, ... (NPAD / 64 of them: conflict-free LDS rows).  Dither, DC
//      removal, raw energy, pre-emphasis (the left neighbour is the previous lane's value: one rotation per register) and the window run
//      in registers, with wave_sum for the two reductions.
//   3. Real FFT as the half-length complex transform of z[m] = x[2m] + i x[2m+1] plus a split step, in float64 (fbank_core.h says why):
//      the windowed frame goes to the wave's LDS buffer, where pairs ARE z; three Stockham passes (FbRadix<NPAD>: radix 8, 8 and NPAD / 128) ping-pong between the wave's two buffers
//      (fbank_core.h), twiddles from the plan's table; the split step writes the power spectrum of bins 0 .. NPAD/2 - 1.
//   4. Lanes take mel filters (lane, lane + 64): a filter is a contiguous bin range, a dot product of <= ~30 terms; log, energy column,
//      (x - mean) * scale, one coalesced row store.
//   5. KIND_MFCC only (ctcn_mfcc; fbank_kernel<NPAD, KIND> is one body for both feature types): stage 4 leaves the log-mel vector in the wave's
//      idle FFT buffer instead of global memory; lane k < num_ceps takes row k of the DCT (table staged bin-major behind the filter table, so
//      consecutive lanes read consecutive words and the log-mel value is a broadcast) in ascending bin order, multiplies by the lifter,
//      applies the energy and HTK column rules and the normalisation, and the wave stores one coalesced row of num_ceps floats.
//   KIND_SPEC (ctcn_spectrogram; the same body): no mel bank; the split step also leaves the Nyquist bin, stage 4 is the log of bins
//      0 .. NPAD/2 with the energy in place of bin 0, lanes storing columns lane, lane + 64, ... of the row of NPAD/2 + 1 floats.
//   Waves of a workgroup never wait for each other after the staging barrier: the FFT buffers are per wave, ordered by wave_lds_sync.
#include <algorithm>
#include <vector>

#include "common.h"
#include "fbank_core.h"

namespace {

constexpr size_t FBANK_LDS_LIMIT = 160 * 1024;     // a CU's LDS; launches beyond 64 KB opt in (Npad = 1024: 99 KB)

// Flat and packed: the kernel fetches its arguments with one 16-dword scalar load.
struct FbankArgs {
  const void *wave;
  const int32_t *lens;
  const float *plan;
  const float *mean, *scale;
  float *feats;
  int32_t *frames;
  uint64_t seed, utt_offset;
  int is_i16, Nmax, Tmax, L, shift, nbins, F, fpw;                  // F: columns of an output row (MFCC: the number of cepstra)
  int snip, remove_dc, use_energy, raw_energy, htk, use_log, use_power, has_floor;
  float preemph, log_floor, dither;
};

// LDS traffic between the lanes of ONE wave: drain the wave's own LDS operations and keep the compiler from moving accesses across.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The frames of workgroup (blockIdx.x, utterance blockIdx.y): the utterance has n samples and Tb frames, the block owns frames [f0, f0 + nf)
// of them; nf <= 0: none.  `count`: the front-end's rule from samples to frames.
struct FrameBlock { int n, Tb, f0, nf; };

template <class Count>
__device__ __forceinline__ FrameBlock frame_block(const int32_t *lens, int Nmax, int Tmax, int fpw, Count count) {
  const int b = blockIdx.y;
  FrameBlock fb;
  fb.n = min(max(lens[b], 0), Nmax);
  fb.Tb = min(count(fb.n), Tmax);
  fb.f0 = blockIdx.x * fpw;
  fb.nf = min(fpw, fb.Tb - fb.f0);
  return fb;
}

// The opening of a spectral kernel: frames[b] from one thread of the utterance, zeros for the block's rows at or beyond Tb (`out`: the
// utterance's Tmax rows of F floats).  The caller returns when nf <= 0 -- the whole workgroup does: a barrier follows.
template <class Count>
__device__ __forceinline__ FrameBlock frame_block_begin(const int32_t *lens, int32_t *frames, float *out, int Nmax, int Tmax, int fpw, int F, Count count) {
  const FrameBlock fb = frame_block(lens, Nmax, Tmax, fpw, count);
  const int b = blockIdx.y, tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) frames[b] = fb.Tb;
  const size_t zend = (size_t)min(fb.f0 + fpw, Tmax) * F;
  for (size_t i = (size_t)max(fb.f0, fb.Tb) * F + tid; i < zend; i += 256) out[i] = 0.f;
  return fb;
}

// The N / 2-point complex transform of the frame the wave's lanes have just written to zA as N doubles (pairs ARE z): three Stockham passes
// ping-pong between the wave's two buffers, each behind a sync of the wave; the transform ends in zB, synced.
template <int N>
__device__ __forceinline__ void wave_rfft(int lane, fbc *zA, fbc *zB, const fbc *tw) {
  constexpr int M = N / 2;
  using Radix = FbRadix<N>;
  wave_lds_sync();
  fbank_fft_pass<M, Radix::r0>(lane, 1, zA, zB, tw);
  wave_lds_sync();
  fbank_fft_pass<M, Radix::r1>(lane, Radix::r0, zB, zA, tw);
  wave_lds_sync();
  fbank_fft_pass<M, Radix::r2>(lane, Radix::r0 * Radix::r1, zA, zB, tw);
  wave_lds_sync();
}

// N(0, 1) for sample i of frame `frame` of utterance `utt`: one Philox call per sample pair, Box-Muller's cosine for the even, sine for the odd one
__device__ __forceinline__ float fbank_gauss(uint64_t seed, uint64_t utt, int frame, int i) {
  uint32_t w[4];
  philox4(seed, (utt << 38) | ((uint64_t)(uint32_t)frame << 10) | (uint64_t)(i >> 1), w);
  const float u1 = ((float)(w[0] >> 8) + 1.0f) * 5.9604644775390625e-08f;      // (0, 1]
  const float th = 6.28318530717958647692f * ((float)(w[1] >> 8) * 5.9604644775390625e-08f);
  const float r = sqrtf(-2.0f * logf(u1));
  return r * ((i & 1) ? sinf(th) : cosf(th));
}

// The energy of the frame a wave holds in registers
template <int P>
__device__ __forceinline__ float frame_energy(const float (&x)[P]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < P; ++j) s += x[j] * x[j];
  return wave_sum(s);
}

// log(max(v, FLT_EPSILON)), Kaldi's guard of every log here; `floored` (the energy columns): no lower than the log of energy_floor, where one is set
__device__ __forceinline__ float guarded_log(float v, bool floored, const FbankArgs &a) {
  float e = logf(fmaxf(v, FLT_EPSILON));
  if (floored && a.has_floor && e < a.log_floor) e = a.log_floor;
  return e;
}

// column `col` of a feature row, normalised where the call has mean and scale
__device__ __forceinline__ void store_feature(float *row, int col, float v, const FbankArgs &a) {
  if (a.mean != nullptr) v = (v - a.mean[col]) * a.scale[col];
  row[col] = v;
}

template <int NPAD, int KIND>
__global__ __launch_bounds__(256) void fbank_kernel(FbankArgs a) {
  constexpr int P = NPAD / 64, M = NPAD / 2;
  constexpr bool MFCC = KIND == KIND_MFCC, SPEC = KIND == KIND_SPEC;
  extern __shared__ __align__(16) double smem_d[];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = a.L, shift = a.shift, F = a.F;
  FbankLds<NPAD> &lds = *reinterpret_cast<FbankLds<NPAD> *>(smem_d);
  float *dct = reinterpret_cast<float *>(&lds + 1), *span = dct + fbank_lds_table(a.nbins, F, KIND);      // behind the head (fbank_core.h)

  float *out = a.feats + (size_t)b * a.Tmax * F;
  const FrameBlock fb = frame_block_begin(a.lens, a.frames, out, a.Nmax, a.Tmax, a.fpw, F,
                                          [&](int n) { return fbank_num_frames(n, L, shift, a.snip); });
  const int n = fb.n, f0 = fb.f0, nf = fb.nf;
  if (nf <= 0) return;                                               // (the whole workgroup: nothing below is reached by a part of it)

  // ---- 1. stage the plan and the samples ---------------------------------------------------------------------------------------------
  {
    const double *p_tw = reinterpret_cast<const double *>(a.plan + NPAD);
    const float *p_tab = a.plan + 5 * NPAD;
    for (int i = tid; i < 2 * NPAD; i += 256) reinterpret_cast<double *>(lds.tw)[i] = p_tw[i];
    for (int i = tid; i < NPAD; i += 256) lds.win[i] = a.plan[i];
    if (!SPEC) {                                                      // (the spectrogram's plan ends behind the twiddles)
      for (int i = tid; i < 3 * FBANK_MAX_BINS; i += 256) lds.ftab[i] = reinterpret_cast<const int *>(p_tab)[i];
      for (int i = tid; i < NPAD; i += 256) lds.wts[i] = p_tab[3 * FBANK_MAX_BINS + i];
    }
    if (MFCC)
      for (int i = tid; i < a.nbins * a.F + a.F; i += 256) dct[i] = p_tab[3 * FBANK_MAX_BINS + NPAD + i];
    const long long s0 = (long long)f0 * shift + (a.snip ? 0 : shift / 2 - L / 2);
    const int span_len = (nf - 1) * shift + L;
    const size_t base = (size_t)b * a.Nmax;
    for (int i = tid; i < span_len; i += 256) {
      long long s = s0 + i;
      while (s < 0 || s >= n) s = s < 0 ? -s - 1 : 2LL * n - 1 - s;    // Kaldi's reflection; n >= 1 here (Tb > 0), and with snip_edges s is inside already
      span[i] = wave_sample(a.wave, a.is_i16, base + s);
    }
  }
  __syncthreads();

  double *bufA = lds.wbuf[wv][0], *bufB = lds.wbuf[wv][1];
  fbc *zA = reinterpret_cast<fbc *>(bufA), *zB = reinterpret_cast<fbc *>(bufB);
  float *pw = reinterpret_cast<float *>(bufA);                      // the power spectrum, once the transform has left bufA
  float *lm = reinterpret_cast<float *>(bufB);                      // MFCC: the log-mel vector, once the split step has read bufB
  const int mel_off = (a.use_energy && !a.htk) ? 1 : 0;

  for (int fi = wv; fi < nf; fi += 4) {
    const int frame = f0 + fi;
    const float *fr = span + fi * shift;
    // ---- 2. the frame in registers ------------------------------------------------------------------------------------------------------
    float x[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = lane + 64 * j;
      x[j] = i < L ? fr[i] : 0.f;
    }
    if (a.dither > 0.f) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int i = lane + 64 * j;
        if (i < L) x[j] += a.dither * fbank_gauss(a.seed, (uint64_t)b + a.utt_offset, frame, i);
      }
    }
    if (a.remove_dc) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) s += x[j];
      const float mean = wave_sum(s) / (float)L;
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (lane + 64 * j < L) x[j] -= mean;
    }
    float energy = 0.f;
    if (a.use_energy && a.raw_energy) energy = frame_energy(x);
    if (a.preemph != 0.f) {
      float rot[P];                                                   // sample i - 1 lives in the previous lane; lane 0 takes lane 63's previous register
#pragma unroll
      for (int j = 0; j < P; ++j) rot[j] = __shfl(x[j], (lane + 63) & 63, 64);
      const float x0 = x[0];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float prev = lane != 0 ? rot[j] : (j == 0 ? x0 : rot[j > 0 ? j - 1 : 0]);
        x[j] -= a.preemph * prev;
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) x[j] *= lds.win[lane + 64 * j];           // 0 from L on: the zero padding
    if (a.use_energy && !a.raw_energy) energy = frame_energy(x);
    // ---- 3. real FFT -> power spectrum ------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < P; ++j) bufA[lane + 64 * j] = (double)x[j];
    wave_rfft<NPAD>(lane, zA, zB, lds.tw);
    for (int k = lane; k < M; k += 64) {
      const double p = fbank_split_power<M>(k, zB, lds.tw);
      pw[k] = (float)(a.use_power ? p : sqrt(p));
    }
    if (SPEC && lane == 0) pw[M] = (float)fbank_nyquist_power(zB);   // the bin no mel filter reads
    wave_lds_sync();
    // ---- 4. mel bank, log, energy, normalisation -------------------------------------------------------------------------------------------
    float *row = out + (size_t)frame * F;
    if (SPEC) {
      // ---- 4'. the spectrogram: the log of every bin, the energy in place of the DC bin; lanes store lane, lane + 64, ... of the row ----------
      for (int c = lane; c < F; c += 64) store_feature(row, c, guarded_log(c ? pw[c] : energy, c == 0, a), a);
      wave_lds_sync();                                                // the next frame overwrites bufA (pw)
      continue;
    }
    for (int m = lane; m < a.nbins; m += 64) {
      const int first = lds.ftab[m], cnt = lds.ftab[FBANK_MAX_BINS + m];
      const float *w = lds.wts + lds.ftab[2 * FBANK_MAX_BINS + m];
      float e = 0.f;
      for (int i = 0; i < cnt; ++i) e += w[i] * pw[first + i];
      if (a.use_log) e = guarded_log(e, false, a);
      if (MFCC) lm[m] = e;
      else store_feature(row, m + mel_off, e, a);
    }
    if (MFCC) {
      // ---- 5. DCT, lifter, energy and HTK column rules: lane k owns cepstrum k ----------------------------------------------------------------
      wave_lds_sync();                                                // stage 4's own sync above sits behind the split step's reads of bufB
      if (lane < F) {
        float c = 0.f;
        for (int i = 0; i < a.nbins; ++i) c = fmaf(dct[i * F + lane], lm[i], c);      // ascending bins: a function of the frame alone
        c = __fmul_rn(c, dct[a.nbins * F + lane]);                    // (never contracted into the normalisation's subtraction)
        int col = lane;
        if (lane == 0 && a.use_energy) c = guarded_log(energy, true, a);
        if (a.htk) {
          if (lane == 0 && !a.use_energy) c = (float)((double)c * 1.41421356237309504880);
          col = lane == 0 ? F - 1 : lane - 1;
        }
        store_feature(row, col, c, a);
      }
    } else if (a.use_energy && lane == 0) {
      store_feature(row, a.htk ? a.nbins : 0, guarded_log(energy, true, a), a);
    }
    wave_lds_sync();                                                  // the next frame overwrites bufA (pw)
  }
}

// ---- the recipe's log-magnitude STFT (ctcn_logspec) -------------------------------------------------------------------------------------------
// logspec_kernel<N>: the filterbank kernel's shape -- one wave per frame, the plan and the sample span of `fpw` (<= 8) neighbouring frames
//   staged once (numpy's reflection and input_scale applied there) -- with P = ceil(N / 64) registers
//   per lane (N = 400: seven, the float64 window padded with zeros to 448), the passes of FbRadix<N>, and the split step's magnitudes going through
//   log1pf straight to the row.  Every lane keeps float64 sums of its values and their squares; wave_sum_d, then wave 0 .. 3 in order: one
//   (sum, sum of squares) per workgroup in ws.
// logspec_finish_kernel: the same grid; every workgroup of an utterance adds the utterance's partials in index order (the same bits in each),
//   forms mean and standard deviation in double, rounds each once; block 0 writes stats, all normalise their own rows in place.
struct LogSpecArgs {
  const void *wave;
  const int32_t *lens;
  const float *plan;
  float *feats;
  int32_t *frames;
  float *stats;
  double *ws;
  int is_i16, Nmax, Tmax, hop, fpw, normalize;
  float in_scale;
};

template <int N>
__global__ __launch_bounds__(256) void logspec_kernel(LogSpecArgs a) {
  constexpr int P = (N + 63) / 64, M = N / 2, F = M + 1;
  extern __shared__ __align__(16) double smem_d[];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hop = a.hop;
  LogSpecLds<N> &lds = *reinterpret_cast<LogSpecLds<N> *>(smem_d);
  float *span = reinterpret_cast<float *>(&lds + 1);                 // behind the head (fbank_core.h)

  float *out = a.feats + (size_t)b * a.Tmax * F;
  const FrameBlock fb = frame_block_begin(a.lens, a.frames, out, a.Nmax, a.Tmax, a.fpw, F, [&](int n) { return logspec_num_frames(n, hop); });
  const int n = fb.n, f0 = fb.f0, nf = fb.nf;
  if (nf <= 0) return;                                               // (the whole workgroup; the finish kernel reads the partials of blocks with frames only)

  {
    const double *p_win = reinterpret_cast<const double *>(a.plan), *p_tw = p_win + 64 * P;
    for (int i = tid; i < 2 * N; i += 256) reinterpret_cast<double *>(lds.tw)[i] = p_tw[i];
    for (int i = tid; i < 64 * P; i += 256) lds.win[i] = p_win[i];
    const long long s0 = (long long)f0 * hop - N / 2;
    const int span_len = (nf - 1) * hop + N;
    const size_t base = (size_t)b * a.Nmax;
    for (int i = tid; i < span_len; i += 256) {
      const long long s = logspec_reflect(s0 + i, n);                // n >= 1 here (Tb > 0)
      span[i] = __fmul_rn(wave_sample(a.wave, a.is_i16, base + s), a.in_scale);
    }
  }
  __syncthreads();

  double *bufA = lds.wbuf[wv][0], *bufB = lds.wbuf[wv][1];
  fbc *zA = reinterpret_cast<fbc *>(bufA), *zB = reinterpret_cast<fbc *>(bufB);
  double sum = 0.0, sq = 0.0;
  for (int fi = wv; fi < nf; fi += 4) {
    const float *fr = span + fi * hop;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = lane + 64 * j;
      if (i < N) bufA[i] = (double)fr[i] * lds.win[i];                    // exact: 24 x 53 bits round once
    }
    wave_rfft<N>(lane, zA, zB, lds.tw);
    float *row = out + (size_t)(f0 + fi) * F;
    for (int k = lane; k < F; k += 64) {
      const double p = k < M ? fbank_split_power<M>(k, zB, lds.tw) : fbank_nyquist_power(zB);
      const float v = log1pf((float)sqrt(p));
      row[k] = v;
      sum += (double)v;
      sq += (double)v * (double)v;
    }
    wave_lds_sync();                                                  // the next frame overwrites bufA and bufB
  }
  sum = wave_sum_d(sum);
  sq = wave_sum_d(sq);
  if (lane == 0) { lds.red[2 * wv] = sum; lds.red[2 * wv + 1] = sq; }
  __syncthreads();
  if (tid < 2) a.ws[((size_t)b * gridDim.x + blockIdx.x) * 2 + tid] = ((lds.red[tid] + lds.red[2 + tid]) + lds.red[4 + tid]) + lds.red[6 + tid];
}

__global__ __launch_bounds__(256) void logspec_finish_kernel(LogSpecArgs a, int F) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const FrameBlock fb = frame_block(a.lens, a.Nmax, a.Tmax, a.fpw, [&](int n) { return logspec_num_frames(n, a.hop); });
  const int Tb = fb.Tb, nb = (Tb + a.fpw - 1) / a.fpw;                // the blocks that left partials
  if ((int)blockIdx.x >= nb && blockIdx.x != 0) return;
  double s = 0.0, q = 0.0;
  for (int p = 0; p < nb; ++p) {                                      // every thread of every block of the utterance: the same sum
    s += a.ws[((size_t)b * gridDim.x + p) * 2];
    q += a.ws[((size_t)b * gridDim.x + p) * 2 + 1];
  }
  float m = 0.f, sd = 0.f;
  if (Tb > 0) {
    const double cnt = (double)Tb * (double)F, mean = s / cnt;
    m = (float)mean;
    sd = (float)sqrt(fmax(q / cnt - mean * mean, 0.0));
  }
  if (blockIdx.x == 0 && tid == 0) { a.stats[2 * b] = m; a.stats[2 * b + 1] = sd; }
  if (!a.normalize || (int)blockIdx.x >= nb) return;
  float *x = a.feats + ((size_t)b * a.Tmax + fb.f0) * F;
  const int cnt = fb.nf * F;                                          // (a block below nb has frames)
  for (int i = tid; i < cnt; i += 256) x[i] = sd > 0.f ? __fdiv_rn(__fsub_rn(x[i], m), sd) : 0.f;
}

// ---- the host side: geometry and plans, frames per workgroup, kernel choice, launch ------------------------------------------------------------

// The geometry of a configuration by `geom` (fbank_geom's kin): CTCN_OK and *g, or the refusal's code with "<who>: <reason>" left as the error
// (who == nullptr: no error text, for the *_plan_bytes functions, which answer 0).
template <class Opts, class Geom>
int config_geom(const char *who, int (*geom)(const Opts *, Geom *, const char **), const Opts *opts, Geom *g) {
  const char *why;
  const int rc = geom(opts, g, &why);
  if (rc != CTCN_OK && who) ctcn_set_error("%s: %s", who, why);
  return rc;
}

template <class Opts, class Geom>
size_t plan_bytes_of(int (*geom)(const Opts *, Geom *, const char **), const Opts *opts) {
  Geom g;
  return config_geom(nullptr, geom, opts, &g) == CTCN_OK ? g.words * 4 : 0;
}

// A ctcn_*_plan entry point: geometry, the size check, then `build(g, &why)` fills the caller's block.
template <class Opts, class Geom, class Build>
int build_plan(const char *who, int (*geom)(const Opts *, Geom *, const char **), const Opts *opts, void *plan, size_t plan_bytes, Build build) {
  Geom g;
  int rc = config_geom(who, geom, opts, &g);
  if (rc != CTCN_OK) return rc;
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4, "%s: buffer of %zu bytes needed", who, g.words * 4);
  const char *why = "";
  rc = build(g, &why);
  if (rc != CTCN_OK) ctcn_set_error("%s: %s", who, why);
  return rc;
}

int fbank_mel_geom(const ctcn_fbank_opts *o, FbankGeom *g, const char **why) { return fbank_geom(o, g, why); }     // (with the mel bank)

// Frames per workgroup: eight where `words(fpw)`, the kernel's LDS layout, fits in a CU's LDS, else halved down to one; 0: not even one frame does.
template <class Words>
int pick_fpw(Words words) {
  for (int fpw = 8; fpw >= 1; fpw >>= 1)
    if (words(fpw) * 4 <= FBANK_LDS_LIMIT) return fpw;
  return 0;
}

size_t logspec_lds_words(const LogSpecGeom &g, int fpw) { return logspec_lds_head(g.nfft) / 4 + lds_samples(fpw, g.hop, g.nfft); }

int logspec_fpw(const LogSpecGeom &g) { return pick_fpw([&](int fpw) { return logspec_lds_words(g, fpw); }); }

// The launch of the three feature types of fbank_kernel: `o` are the filterbank options stages 1-4 run with, F the columns of an output row.
int fbank_launch(const char *who, int kind, const ctcn_fbank_opts *o, const FbankGeom &g, int F, const void *wave, int wave_is_int16,
                 const int32_t *lens, const void *plan, const float *mean, const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax,
                 float dither, uint64_t seed, uint64_t utt_offset, void *stream) {
  CTCN_REQUIRE(lens && plan && frames && B > 0 && Nmax >= 0 && Tmax >= 0 && (wave || Nmax == 0) && (feats || Tmax == 0), "%s: bad args", who);
  CTCN_REQUIRE((mean == nullptr) == (scale == nullptr), "%s: mean and scale come together", who);
  CTCN_REQUIRE(dither >= 0.f && B <= 65535, "%s: dither must not be negative, B at most 65 535 per call (B %d)", who, B);
  const auto words = [&](int fpw) { return fbank_lds_head(g.npad) / 4 + fbank_lds_table(g.nbins, F, kind) + lds_samples(fpw, g.shift, g.L); };
  const int fpw = pick_fpw(words);
  if (!fpw) { ctcn_set_error("%s: frame shift %d too long for the LDS staging", who, g.shift); return CTCN_EUNSUPPORTED; }
  FbankArgs a;
  a.wave = wave; a.lens = lens; a.plan = static_cast<const float *>(plan); a.mean = mean; a.scale = scale; a.feats = feats; a.frames = frames;
  a.seed = seed; a.utt_offset = utt_offset;
  a.is_i16 = wave_is_int16 != 0; a.Nmax = Nmax; a.Tmax = Tmax; a.L = g.L; a.shift = g.shift; a.nbins = g.nbins; a.F = F; a.fpw = fpw;
  a.snip = o->snip_edges != 0; a.remove_dc = o->remove_dc_offset != 0; a.use_energy = o->use_energy != 0; a.raw_energy = o->raw_energy != 0;
  a.htk = o->htk_compat != 0; a.use_log = o->use_log_fbank != 0; a.use_power = o->use_power != 0;
  a.has_floor = o->energy_floor > 0.f; a.log_floor = a.has_floor ? logf(o->energy_floor) : 0.f;
  a.preemph = o->preemph_coeff; a.dither = dither;
  const size_t lds = words(fpw) * 4;
  void (*kern)(FbankArgs);
  if (kind == KIND_SPEC) kern = g.npad == 256 ? fbank_kernel<256, KIND_SPEC> : g.npad == 512 ? fbank_kernel<512, KIND_SPEC> : fbank_kernel<1024, KIND_SPEC>;
  else if (kind == KIND_MFCC) kern = g.npad == 256 ? fbank_kernel<256, KIND_MFCC> : g.npad == 512 ? fbank_kernel<512, KIND_MFCC> : fbank_kernel<1024, KIND_MFCC>;
  else kern = g.npad == 256 ? fbank_kernel<256, KIND_FBANK> : g.npad == 512 ? fbank_kernel<512, KIND_FBANK> : fbank_kernel<1024, KIND_FBANK>;
  if (lds > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(std::max(ceil_div(Tmax, fpw), 1), B), dim3(256), lds, (hipStream_t)stream, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

}  // namespace

extern "C" int ctcn_fbank_frames(long long num_samples, int frame_length, int frame_shift, int snip_edges) {
  CTCN_REQUIRE(num_samples >= 0 && frame_length > 0 && frame_shift > 0, "ctcn_fbank_frames: bad args (samples %lld, frame length %d, shift %d)",
               num_samples, frame_length, frame_shift);
  CTCN_REQUIRE((num_samples + frame_shift / 2) / frame_shift < 0x7fffffffLL, "ctcn_fbank_frames: frame count beyond int");
  return fbank_num_frames(num_samples, frame_length, frame_shift, snip_edges);
}

extern "C" size_t ctcn_fbank_plan_bytes(const ctcn_fbank_opts *opts) { return plan_bytes_of(fbank_mel_geom, opts); }

extern "C" int ctcn_fbank_plan(const ctcn_fbank_opts *opts, void *plan, size_t plan_bytes) {
  return build_plan("ctcn_fbank_plan", fbank_mel_geom, opts, plan, plan_bytes,
                    [&](const FbankGeom &g, const char **why) { return fbank_build_plan(opts, g, plan, why); });
}

extern "C" int ctcn_fbank(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_fbank_opts *opts, const void *plan, const float *mean,
                          const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed,
                          uint64_t utt_offset, void *stream) {
  FbankGeom g;
  const int rc = config_geom("ctcn_fbank", fbank_mel_geom, opts, &g);
  if (rc != CTCN_OK) return rc;
  return fbank_launch("ctcn_fbank", KIND_FBANK, opts, g, g.F, wave, wave_is_int16, lens, plan, mean, scale, feats, frames, B, Nmax, Tmax, dither, seed,
                      utt_offset, stream);
}

extern "C" size_t ctcn_mfcc_plan_bytes(const ctcn_mfcc_opts *opts) { return plan_bytes_of(mfcc_geom, opts); }

extern "C" int ctcn_mfcc_plan(const ctcn_mfcc_opts *opts, void *plan, size_t plan_bytes) {
  return build_plan("ctcn_mfcc_plan", mfcc_geom, opts, plan, plan_bytes,
                    [&](const MfccGeom &g, const char **why) { return mfcc_build_plan(opts, g, plan, why); });
}

extern "C" int ctcn_mfcc(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_mfcc_opts *opts, const void *plan, const float *mean,
                         const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed,
                         uint64_t utt_offset, void *stream) {
  MfccGeom g;
  const int rc = config_geom("ctcn_mfcc", mfcc_geom, opts, &g);
  if (rc != CTCN_OK) return rc;
  const ctcn_fbank_opts f = mfcc_fbank_opts(opts);
  return fbank_launch("ctcn_mfcc", KIND_MFCC, &f, g.fb, g.nceps, wave, wave_is_int16, lens, plan, mean, scale, feats, frames, B, Nmax, Tmax, dither, seed,
                      utt_offset, stream);
}

extern "C" size_t ctcn_spectrogram_plan_bytes(const ctcn_spectrogram_opts *opts) { return plan_bytes_of(spectrogram_geom, opts); }

extern "C" int ctcn_spectrogram_plan(const ctcn_spectrogram_opts *opts, void *plan, size_t plan_bytes) {
  return build_plan("ctcn_spectrogram_plan", spectrogram_geom, opts, plan, plan_bytes, [&](const FbankGeom &g, const char **) {
    const ctcn_fbank_opts f = spectrogram_fbank_opts(opts);
    fbank_build_window(&f, g, plan);
    return CTCN_OK;
  });
}

extern "C" int ctcn_spectrogram(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_spectrogram_opts *opts, const void *plan,
                                const float *mean, const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither,
                                uint64_t seed, uint64_t utt_offset, void *stream) {
  FbankGeom g;
  const int rc = config_geom("ctcn_spectrogram", spectrogram_geom, opts, &g);
  if (rc != CTCN_OK) return rc;
  const ctcn_fbank_opts f = spectrogram_fbank_opts(opts);
  return fbank_launch("ctcn_spectrogram", KIND_SPEC, &f, g, g.F, wave, wave_is_int16, lens, plan, mean, scale, feats, frames, B, Nmax, Tmax, dither, seed,
                      utt_offset, stream);
}

extern "C" int ctcn_logspec_frames(long long num_samples, int hop) {
  CTCN_REQUIRE(num_samples >= 0 && hop > 0, "ctcn_logspec_frames: bad args (samples %lld, hop %d)", num_samples, hop);
  CTCN_REQUIRE(num_samples / hop < 0x7ffffffeLL, "ctcn_logspec_frames: frame count beyond int");
  return logspec_num_frames(num_samples, hop);
}

extern "C" size_t ctcn_logspec_plan_bytes(const ctcn_logspec_opts *opts) { return plan_bytes_of(logspec_geom, opts); }

extern "C" int ctcn_logspec_plan(const ctcn_logspec_opts *opts, void *plan, size_t plan_bytes) {
  return build_plan("ctcn_logspec_plan", logspec_geom, opts, plan, plan_bytes, [&](const LogSpecGeom &g, const char **) {
    logspec_build_plan(opts, g, plan);
    return CTCN_OK;
  });
}

extern "C" size_t ctcn_logspec_ws_bytes(const ctcn_logspec_opts *opts, int B, int Tmax) {
  LogSpecGeom g;
  if (config_geom(nullptr, logspec_geom, opts, &g) != CTCN_OK || B <= 0 || Tmax < 0) return 0;
  const int fpw = logspec_fpw(g);
  return fpw ? (size_t)B * std::max(ceil_div(Tmax, fpw), 1) * 2 * sizeof(double) : 0;
}

extern "C" int ctcn_logspec(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_logspec_opts *opts, const void *plan, float *feats,
                            int32_t *frames, float *stats, int B, int Nmax, int Tmax, void *ws, size_t ws_bytes, void *stream) {
  LogSpecGeom g;
  const int rc = config_geom("ctcn_logspec", logspec_geom, opts, &g);
  if (rc != CTCN_OK) return rc;
  CTCN_REQUIRE(lens && plan && frames && stats && B > 0 && B <= 65535 && Nmax >= 0 && Tmax >= 0 && (wave || Nmax == 0) && (feats || Tmax == 0),
               "ctcn_logspec: bad args (B %d at most 65 535)", B);
  const int fpw = logspec_fpw(g);
  if (!fpw) { ctcn_set_error("ctcn_logspec: window stride of %d samples too long for the LDS staging", g.hop); return CTCN_EUNSUPPORTED; }
  const size_t need = ctcn_logspec_ws_bytes(opts, B, Tmax);
  CTCN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "ctcn_logspec: workspace of ctcn_logspec_ws_bytes needed, 8-byte aligned");
  if (ws_bytes < need) { ctcn_set_error("ctcn_logspec: workspace %zu < %zu bytes", ws_bytes, need); return CTCN_EWORKSPACE; }
  LogSpecArgs a;
  a.wave = wave; a.lens = lens; a.plan = static_cast<const float *>(plan); a.feats = feats; a.frames = frames; a.stats = stats;
  a.ws = static_cast<double *>(ws);
  a.is_i16 = wave_is_int16 != 0; a.Nmax = Nmax; a.Tmax = Tmax; a.hop = g.hop; a.fpw = fpw; a.normalize = opts->normalize != 0;
  a.in_scale = opts->input_scale;
  const dim3 grid(std::max(ceil_div(Tmax, fpw), 1), B);
  const size_t lds = logspec_lds_words(g, fpw) * 4;
  hipStream_t st = (hipStream_t)stream;
  void (*kern)(LogSpecArgs) = g.nfft == 256 ? logspec_kernel<256> : g.nfft == 400 ? logspec_kernel<400> : g.nfft == 512 ? logspec_kernel<512> : logspec_kernel<1024>;
  if (lds > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
  CTCN_LAUNCH_CHECK();
  hipLaunchKernelGGL(logspec_finish_kernel, grid, dim3(256), 0, st, a, g.F);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_fbank_power_host(const double *frame, int n, double *power) {
  CTCN_REQUIRE(frame && power, "ctcn_fbank_power_host: null argument");
  if (n != 256 && n != 400 && n != 512 && n != 1024) { ctcn_set_error("ctcn_fbank_power_host: n must be 256, 400, 512 or 1024, got %d", n); return CTCN_EUNSUPPORTED; }
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<fbc> buf(n), tw(n);                                      // a | b of n / 2 complex each
  for (int k = 0; k < n; ++k) tw[k] = fb_c(cos(two_pi * k / n), -sin(two_pi * k / n));
  memcpy(buf.data(), frame, sizeof(double) * n);                      // pairs ARE z[m] = x[2m] + i x[2m+1]
  fbc *za = buf.data(), *zb = za + n / 2;
  switch (n) {
    case 256: fbank_power_host<256>(za, zb, tw.data(), power); break;
    case 400: fbank_power_host<400>(za, zb, tw.data(), power); break;
    case 512: fbank_power_host<512>(za, zb, tw.data(), power); break;
    default: fbank_power_host<1024>(za, zb, tw.data(), power); break;
  }
  return CTCN_OK;
}
