// fbank.hip -- the filterbank front-end: waveform -> (normalised) log-mel features, and the statistics of the global mean / variance
// normalisation (ctcn_fbank_frames, ctcn_fbank_plan, ctcn_fbank, ctcn_mfcc_plan, ctcn_mfcc, ctcn_cmvn_accumulate; contract and plan layouts in
// include/ctcn.h); Kaldi's spectrogram by the same kernel (ctcn_spectrogram) and the recipe's log-magnitude STFT with its per-utterance
// normalisation (ctcn_logspec: logspec_kernel / logspec_finish_kernel below); ctcn_fbank_power_host, the transform on the host.
//
// fbank_kernel<NPAD, KIND>: grid (frame blocks, utterances), four waves per workgroup.
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
//   Rows of the block at or beyond the utterance's frame count are zero-filled by the whole workgroup first.
//   Waves of a workgroup never wait for each other after the staging barrier: the FFT buffers are per wave, ordered by wave_lds_sync.
// cmvn_partial_kernel / cmvn_finish_kernel: float64 column sums of 64-row blocks into the workspace, then one thread per statistic adds the
//   partials in index order into the caller's block (norm.hip's scheme: no atomics, a function of the input bits).
//   cmvn_finish_groups_kernel: the second step per group of utterances (ctcn_cmvn_accumulate_groups; the apply side is cmvn.hip).
#include <algorithm>
#include <vector>

#include "common.h"
#include "fbank_core.h"

namespace {

constexpr size_t FBANK_LDS_LIMIT = 160 * 1024;     // a CU's LDS; launches beyond 64 KB opt in (Npad = 1024: 99 KB)
constexpr int CMVN_ROWS = 64;

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

// `extra`: the words of the plan behind the filterbank block (MFCC: DCT table and lifter), staged between the filter table and the samples
static inline size_t fbank_lds_words(int npad, int L, int shift, int fpw, int extra) {
  return (size_t)22 * npad + 3 * FBANK_MAX_BINS + extra + (size_t)(fpw - 1) * shift + L;      // 4-byte words: twiddles 4, wave buffers 16, window 1, weights 1 (x npad)
}

// LDS traffic between the lanes of ONE wave: drain the wave's own LDS operations and keep the compiler from moving accesses across.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
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

enum { KIND_FBANK = 0, KIND_MFCC = 1, KIND_SPEC = 2 };

template <int NPAD, int KIND>
__global__ __launch_bounds__(256) void fbank_kernel(FbankArgs a) {
  constexpr int P = NPAD / 64, M = NPAD / 2;
  constexpr bool MFCC = KIND == KIND_MFCC, SPEC = KIND == KIND_SPEC;
  using Radix = FbRadix<NPAD>;
  extern __shared__ __align__(16) double smem_d[];
  fbc *tw = reinterpret_cast<fbc *>(smem_d);                        // NPAD complex doubles
  double *wbuf = smem_d + 2 * NPAD;                                 // 4 waves x 2 x NPAD doubles (M complex each)
  float *win = reinterpret_cast<float *>(wbuf + 8 * NPAD);          // NPAD
  float *wts = win + NPAD;                                          // NPAD
  int *ftab = reinterpret_cast<int *>(wts + NPAD);                  // first | count | weight offset, 128 each
  float *dct = wts + NPAD + 3 * FBANK_MAX_BINS;                     // MFCC: nbins x F bin-major, then the lifter (F)
  float *span = dct + (MFCC ? a.nbins * a.F + a.F : 0);

  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = a.L, shift = a.shift, F = a.F;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const int Tb = min(fbank_num_frames(n, L, shift, a.snip), a.Tmax);
  if (blockIdx.x == 0 && tid == 0) a.frames[b] = Tb;
  const int f0 = blockIdx.x * a.fpw;
  float *out = a.feats + (size_t)b * a.Tmax * F;
  {
    const size_t zend = (size_t)min(f0 + a.fpw, a.Tmax) * F;
    for (size_t i = (size_t)max(f0, Tb) * F + tid; i < zend; i += 256) out[i] = 0.f;
  }
  const int nf = min(a.fpw, Tb - f0);
  if (nf <= 0) return;                                               // (the whole workgroup: nothing below is reached by a part of it)

  // ---- 1. stage the plan and the samples ---------------------------------------------------------------------------------------------
  {
    const double *p_tw = reinterpret_cast<const double *>(a.plan + NPAD);
    const float *p_tab = a.plan + 5 * NPAD;
    for (int i = tid; i < 2 * NPAD; i += 256) smem_d[i] = p_tw[i];
    for (int i = tid; i < NPAD; i += 256) win[i] = a.plan[i];
    if (!SPEC) {                                                      // (the spectrogram's plan ends behind the twiddles)
      for (int i = tid; i < 3 * FBANK_MAX_BINS; i += 256) ftab[i] = reinterpret_cast<const int *>(p_tab)[i];
      for (int i = tid; i < NPAD; i += 256) wts[i] = p_tab[3 * FBANK_MAX_BINS + i];
    }
    if (MFCC)
      for (int i = tid; i < a.nbins * a.F + a.F; i += 256) dct[i] = p_tab[3 * FBANK_MAX_BINS + NPAD + i];
    const long long s0 = (long long)f0 * shift + (a.snip ? 0 : shift / 2 - L / 2);
    const int span_len = (nf - 1) * shift + L;
    const size_t base = (size_t)b * a.Nmax;
    for (int i = tid; i < span_len; i += 256) {
      long long s = s0 + i;
      while (s < 0 || s >= n) s = s < 0 ? -s - 1 : 2LL * n - 1 - s;    // Kaldi's reflection; n >= 1 here (Tb > 0), and with snip_edges s is inside already
      span[i] = a.is_i16 ? (float)static_cast<const int16_t *>(a.wave)[base + s] : static_cast<const float *>(a.wave)[base + s];
    }
  }
  __syncthreads();

  double *bufA = wbuf + wv * 2 * NPAD, *bufB = bufA + NPAD;
  fbc *zA = reinterpret_cast<fbc *>(bufA), *zB = reinterpret_cast<fbc *>(bufB);
  float *pw = reinterpret_cast<float *>(bufA);                      // the power spectrum, once the transform has left bufA
  float *lm = reinterpret_cast<float *>(bufB);                      // MFCC: the log-mel vector, once the split step has read bufB
  const int mel_off = (a.use_energy && !a.htk) ? 1 : 0;
  const bool norm = a.mean != nullptr;

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
    if (a.use_energy && a.raw_energy) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) s += x[j] * x[j];
      energy = wave_sum(s);
    }
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
    for (int j = 0; j < P; ++j) x[j] *= win[lane + 64 * j];           // 0 from L on: the zero padding
    if (a.use_energy && !a.raw_energy) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) s += x[j] * x[j];
      energy = wave_sum(s);
    }
    // ---- 3. real FFT -> power spectrum ------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < P; ++j) bufA[lane + 64 * j] = (double)x[j];
    wave_lds_sync();
    fbank_fft_pass<M, Radix::r0>(lane, 1, zA, zB, tw);
    wave_lds_sync();
    fbank_fft_pass<M, Radix::r1>(lane, Radix::r0, zB, zA, tw);
    wave_lds_sync();
    fbank_fft_pass<M, Radix::r2>(lane, Radix::r0 * Radix::r1, zA, zB, tw);
    wave_lds_sync();
    for (int k = lane; k < M; k += 64) {
      const double p = fbank_split_power<M>(k, zB, tw);
      pw[k] = (float)(a.use_power ? p : sqrt(p));
    }
    if (SPEC && lane == 0) pw[M] = (float)fbank_nyquist_power(zB);   // the bin no mel filter reads
    wave_lds_sync();
    // ---- 4. mel bank, log, energy, normalisation -------------------------------------------------------------------------------------------
    float *row = out + (size_t)frame * F;
    if (SPEC) {
      // ---- 4'. the spectrogram: the log of every bin, the energy in place of the DC bin; lanes store lane, lane + 64, ... of the row ----------
      for (int c = lane; c < F; c += 64) {
        float e = logf(fmaxf(c ? pw[c] : energy, FLT_EPSILON));
        if (c == 0 && a.has_floor && e < a.log_floor) e = a.log_floor;
        if (norm) e = (e - a.mean[c]) * a.scale[c];
        row[c] = e;
      }
      wave_lds_sync();                                                // the next frame overwrites bufA (pw)
      continue;
    }
    for (int m = lane; m < a.nbins; m += 64) {
      const int first = ftab[m], cnt = ftab[FBANK_MAX_BINS + m];
      const float *w = wts + ftab[2 * FBANK_MAX_BINS + m];
      float e = 0.f;
      for (int i = 0; i < cnt; ++i) e += w[i] * pw[first + i];
      if (a.use_log) e = logf(fmaxf(e, FLT_EPSILON));
      if (MFCC) { lm[m] = e; continue; }
      const int col = m + mel_off;
      if (norm) e = (e - a.mean[col]) * a.scale[col];
      row[col] = e;
    }
    if (MFCC) {
      // ---- 5. DCT, lifter, energy and HTK column rules: lane k owns cepstrum k ----------------------------------------------------------------
      wave_lds_sync();                                                // stage 4's own sync above sits behind the split step's reads of bufB
      if (lane < F) {
        float c = 0.f;
        for (int i = 0; i < a.nbins; ++i) c = fmaf(dct[i * F + lane], lm[i], c);      // ascending bins: a function of the frame alone
        c = __fmul_rn(c, dct[a.nbins * F + lane]);                    // (never contracted into the normalisation's subtraction)
        int col = lane;
        if (lane == 0 && a.use_energy) {
          c = logf(fmaxf(energy, FLT_EPSILON));
          if (a.has_floor && c < a.log_floor) c = a.log_floor;
        }
        if (a.htk) {
          if (lane == 0 && !a.use_energy) c = (float)((double)c * 1.41421356237309504880);
          col = lane == 0 ? F - 1 : lane - 1;
        }
        if (norm) c = (c - a.mean[col]) * a.scale[col];
        row[col] = c;
      }
    } else if (a.use_energy && lane == 0) {
      float le = logf(fmaxf(energy, FLT_EPSILON));
      if (a.has_floor && le < a.log_floor) le = a.log_floor;
      const int col = a.htk ? a.nbins : 0;
      if (norm) le = (le - a.mean[col]) * a.scale[col];
      row[col] = le;
    }
    wave_lds_sync();                                                  // the next frame overwrites bufA (pw)
  }
}

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

// thread i < 2F adds its column of the partials in index order into stats; thread 2F adds the frame count
__global__ __launch_bounds__(256) void cmvn_finish_kernel(const double *__restrict__ ws, const int32_t *__restrict__ frames, double *__restrict__ stats,
                                                          int B, int Tmax, int F, int chunks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 2 * F) {
    double s = 0.0;
    for (size_t p = 0; p < (size_t)B * chunks; ++p) s += ws[p * 2 * F + i];
    stats[i < F ? i : i + 1] += s;                                    // row 1 starts at F + 1
  } else if (i == 2 * F) {
    double cnt = 0.0;
    for (int b = 0; b < B; ++b) cnt += (double)min(max(frames[b], 0), Tmax);
    stats[F] += cnt;
  }
}

// The same sums per group of utterances (ctcn_cmvn_accumulate_groups): grid (statistics / 256, groups).  Thread i < 2F of group g adds its
// column of the partials of the utterances with group[b] == g, in ascending (utterance, block) order, into stats[g]; thread 2F their frame
// counts in ascending utterance order.  One group holding every utterance: cmvn_finish_kernel's additions in cmvn_finish_kernel's order.
__global__ __launch_bounds__(256) void cmvn_finish_groups_kernel(const double *__restrict__ ws, const int32_t *__restrict__ frames,
                                                                 const int32_t *__restrict__ group, double *__restrict__ stats, int B, int Tmax, int F,
                                                                 int chunks) {
  const int i = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  double *st = stats + (size_t)g * 2 * (F + 1);
  if (i < 2 * F) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      if (group[b] != g) continue;
      const double *p = ws + (size_t)b * chunks * 2 * F + i;
#pragma unroll 8
      for (int c = 0; c < chunks; ++c) s += p[(size_t)c * 2 * F];   // the loads do not wait for the sum: eight in flight, added in order
    }
    st[i < F ? i : i + 1] += s;
  } else if (i == 2 * F) {
    double cnt = 0.0;
    for (int b = 0; b < B; ++b)
      if (group[b] == g) cnt += (double)min(max(frames[b], 0), Tmax);
    st[F] += cnt;
  }
}

// ---- the recipe's log-magnitude STFT (ctcn_logspec) -------------------------------------------------------------------------------------------
// logspec_kernel<N>: the filterbank kernel's shape -- grid (frame blocks, utterances), four waves, one wave per frame, the plan and the sample
//   span of `fpw` (<= 8) neighbouring frames staged once (numpy's reflection and input_scale applied there) -- with P = ceil(N / 64) registers
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

static inline size_t logspec_lds_words(int nfft, int wpad, int hop, int fpw) {
  return (size_t)20 * nfft + 16 + 2 * wpad + (size_t)(fpw - 1) * hop + nfft;     // 4-byte words: twiddles 4, wave buffers 16 (x nfft), 8 doubles of partial sums, float64 window, samples
}

template <int N>
__global__ __launch_bounds__(256) void logspec_kernel(LogSpecArgs a) {
  constexpr int P = (N + 63) / 64, M = N / 2, F = M + 1;
  using Radix = FbRadix<N>;
  extern __shared__ __align__(16) double smem_d[];
  fbc *tw = reinterpret_cast<fbc *>(smem_d);                        // N complex doubles
  double *wbuf = smem_d + 2 * N;                                    // 4 waves x 2 x N doubles (M complex each)
  double *red = wbuf + 8 * N;                                       // 4 waves x (sum, sum of squares)
  double *win = red + 8;                                            // 64 P
  float *span = reinterpret_cast<float *>(win + 64 * P);

  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hop = a.hop;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const int Tb = min(logspec_num_frames(n, hop), a.Tmax);
  if (blockIdx.x == 0 && tid == 0) a.frames[b] = Tb;
  const int f0 = blockIdx.x * a.fpw;
  float *out = a.feats + (size_t)b * a.Tmax * F;
  {
    const size_t zend = (size_t)min(f0 + a.fpw, a.Tmax) * F;
    for (size_t i = (size_t)max(f0, Tb) * F + tid; i < zend; i += 256) out[i] = 0.f;
  }
  const int nf = min(a.fpw, Tb - f0);
  if (nf <= 0) return;                                               // (the whole workgroup; the finish kernel reads the partials of blocks with frames only)

  {
    const double *p_win = reinterpret_cast<const double *>(a.plan), *p_tw = p_win + 64 * P;
    for (int i = tid; i < 2 * N; i += 256) smem_d[i] = p_tw[i];
    for (int i = tid; i < 64 * P; i += 256) win[i] = p_win[i];
    const long long s0 = (long long)f0 * hop - N / 2;
    const int span_len = (nf - 1) * hop + N;
    const size_t base = (size_t)b * a.Nmax;
    for (int i = tid; i < span_len; i += 256) {
      const long long s = logspec_reflect(s0 + i, n);                // n >= 1 here (Tb > 0)
      const float v = a.is_i16 ? (float)static_cast<const int16_t *>(a.wave)[base + s] : static_cast<const float *>(a.wave)[base + s];
      span[i] = __fmul_rn(v, a.in_scale);
    }
  }
  __syncthreads();

  double *bufA = wbuf + wv * 2 * N, *bufB = bufA + N;
  fbc *zA = reinterpret_cast<fbc *>(bufA), *zB = reinterpret_cast<fbc *>(bufB);
  double sum = 0.0, sq = 0.0;
  for (int fi = wv; fi < nf; fi += 4) {
    const float *fr = span + fi * hop;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = lane + 64 * j;
      if (i < N) bufA[i] = (double)fr[i] * win[i];                    // exact: 24 x 53 bits round once
    }
    wave_lds_sync();
    fbank_fft_pass<M, Radix::r0>(lane, 1, zA, zB, tw);
    wave_lds_sync();
    fbank_fft_pass<M, Radix::r1>(lane, Radix::r0, zB, zA, tw);
    wave_lds_sync();
    fbank_fft_pass<M, Radix::r2>(lane, Radix::r0 * Radix::r1, zA, zB, tw);
    wave_lds_sync();
    float *row = out + (size_t)(f0 + fi) * F;
    for (int k = lane; k < F; k += 64) {
      const double p = k < M ? fbank_split_power<M>(k, zB, tw) : fbank_nyquist_power(zB);
      const float v = log1pf((float)sqrt(p));
      row[k] = v;
      sum += (double)v;
      sq += (double)v * (double)v;
    }
    wave_lds_sync();                                                  // the next frame overwrites bufA and bufB
  }
  sum = wave_sum_d(sum);
  sq = wave_sum_d(sq);
  if (lane == 0) { red[2 * wv] = sum; red[2 * wv + 1] = sq; }
  __syncthreads();
  if (tid < 2) a.ws[((size_t)b * gridDim.x + blockIdx.x) * 2 + tid] = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
}

__global__ __launch_bounds__(256) void logspec_finish_kernel(LogSpecArgs a, int F) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(a.lens[b], 0), a.Nmax);
  const int Tb = min(logspec_num_frames(n, a.hop), a.Tmax);
  const int nb = (Tb + a.fpw - 1) / a.fpw;                           // the blocks that left partials
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
  const int f0 = blockIdx.x * a.fpw;
  float *x = a.feats + ((size_t)b * a.Tmax + f0) * F;
  const int cnt = (min(f0 + a.fpw, Tb) - f0) * F;
  for (int i = tid; i < cnt; i += 256) x[i] = sd > 0.f ? __fdiv_rn(__fsub_rn(x[i], m), sd) : 0.f;
}

}  // namespace

extern "C" int ctcn_fbank_frames(long long num_samples, int frame_length, int frame_shift, int snip_edges) {
  CTCN_REQUIRE(num_samples >= 0 && frame_length > 0 && frame_shift > 0, "ctcn_fbank_frames: bad args (samples %lld, frame length %d, shift %d)",
               num_samples, frame_length, frame_shift);
  CTCN_REQUIRE((num_samples + frame_shift / 2) / frame_shift < 0x7fffffffLL, "ctcn_fbank_frames: frame count beyond int");
  return fbank_num_frames(num_samples, frame_length, frame_shift, snip_edges);
}

extern "C" size_t ctcn_fbank_plan_bytes(const ctcn_fbank_opts *opts) {
  FbankGeom g;
  const char *why;
  return fbank_geom(opts, &g, &why) == CTCN_OK ? g.words * 4 : 0;
}

extern "C" int ctcn_fbank_plan(const ctcn_fbank_opts *opts, void *plan, size_t plan_bytes) {
  FbankGeom g;
  const char *why;
  int rc = fbank_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_fbank_plan: %s", why); return rc; }
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4, "ctcn_fbank_plan: buffer of %zu bytes needed", g.words * 4);
  rc = fbank_build_plan(opts, g, plan, &why);
  if (rc != CTCN_OK) ctcn_set_error("ctcn_fbank_plan: %s", why);
  return rc;
}

// The launch of either feature type: `o` are the filterbank options stages 1-4 run with, F the columns of an output row, `extra` the words of
// the plan behind the filterbank block (KIND_MFCC: table and lifter).
static int fbank_launch(const char *who, int kind, const ctcn_fbank_opts *o, const FbankGeom &g, int F, int extra, const void *wave, int wave_is_int16,
                        const int32_t *lens, const void *plan, const float *mean, const float *scale, float *feats, int32_t *frames, int B, int Nmax,
                        int Tmax, float dither, uint64_t seed, uint64_t utt_offset, void *stream) {
  CTCN_REQUIRE(lens && plan && frames && B > 0 && Nmax >= 0 && Tmax >= 0 && (wave || Nmax == 0) && (feats || Tmax == 0), "%s: bad args", who);
  CTCN_REQUIRE((mean == nullptr) == (scale == nullptr), "%s: mean and scale come together", who);
  CTCN_REQUIRE(dither >= 0.f && B <= 65535, "%s: dither must not be negative, B at most 65 535 per call (B %d)", who, B);
  int fpw = 8;
  while (fpw > 1 && fbank_lds_words(g.npad, g.L, g.shift, fpw, extra) * 4 > FBANK_LDS_LIMIT) fpw >>= 1;
  const size_t lds = fbank_lds_words(g.npad, g.L, g.shift, fpw, extra) * 4;
  if (lds > FBANK_LDS_LIMIT) { ctcn_set_error("%s: frame shift %d too long for the LDS staging", who, g.shift); return CTCN_EUNSUPPORTED; }
  FbankArgs a;
  a.wave = wave; a.lens = lens; a.plan = static_cast<const float *>(plan); a.mean = mean; a.scale = scale; a.feats = feats; a.frames = frames;
  a.seed = seed; a.utt_offset = utt_offset;
  a.is_i16 = wave_is_int16 != 0; a.Nmax = Nmax; a.Tmax = Tmax; a.L = g.L; a.shift = g.shift; a.nbins = g.nbins; a.F = F; a.fpw = fpw;
  a.snip = o->snip_edges != 0; a.remove_dc = o->remove_dc_offset != 0; a.use_energy = o->use_energy != 0; a.raw_energy = o->raw_energy != 0;
  a.htk = o->htk_compat != 0; a.use_log = o->use_log_fbank != 0; a.use_power = o->use_power != 0;
  a.has_floor = o->energy_floor > 0.f; a.log_floor = a.has_floor ? logf(o->energy_floor) : 0.f;
  a.preemph = o->preemph_coeff; a.dither = dither;
  const dim3 grid(std::max(ceil_div(Tmax, fpw), 1), B);
  hipStream_t st = (hipStream_t)stream;
  void (*kern)(FbankArgs);
  if (kind == KIND_SPEC) kern = g.npad == 256 ? fbank_kernel<256, KIND_SPEC> : g.npad == 512 ? fbank_kernel<512, KIND_SPEC> : fbank_kernel<1024, KIND_SPEC>;
  else if (kind == KIND_MFCC) kern = g.npad == 256 ? fbank_kernel<256, KIND_MFCC> : g.npad == 512 ? fbank_kernel<512, KIND_MFCC> : fbank_kernel<1024, KIND_MFCC>;
  else kern = g.npad == 256 ? fbank_kernel<256, KIND_FBANK> : g.npad == 512 ? fbank_kernel<512, KIND_FBANK> : fbank_kernel<1024, KIND_FBANK>;
  if (lds > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_fbank(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_fbank_opts *opts, const void *plan, const float *mean,
                          const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed,
                          uint64_t utt_offset, void *stream) {
  FbankGeom g;
  const char *why;
  const int rc = fbank_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_fbank: %s", why); return rc; }
  return fbank_launch("ctcn_fbank", KIND_FBANK, opts, g, g.F, 0, wave, wave_is_int16, lens, plan, mean, scale, feats, frames, B, Nmax, Tmax, dither, seed,
                      utt_offset, stream);
}

extern "C" size_t ctcn_mfcc_plan_bytes(const ctcn_mfcc_opts *opts) {
  MfccGeom g;
  const char *why;
  return mfcc_geom(opts, &g, &why) == CTCN_OK ? g.words * 4 : 0;
}

extern "C" int ctcn_mfcc_plan(const ctcn_mfcc_opts *opts, void *plan, size_t plan_bytes) {
  MfccGeom g;
  const char *why;
  int rc = mfcc_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_mfcc_plan: %s", why); return rc; }
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4, "ctcn_mfcc_plan: buffer of %zu bytes needed", g.words * 4);
  rc = mfcc_build_plan(opts, g, plan, &why);
  if (rc != CTCN_OK) ctcn_set_error("ctcn_mfcc_plan: %s", why);
  return rc;
}

extern "C" int ctcn_mfcc(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_mfcc_opts *opts, const void *plan, const float *mean,
                         const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed,
                         uint64_t utt_offset, void *stream) {
  MfccGeom g;
  const char *why;
  const int rc = mfcc_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_mfcc: %s", why); return rc; }
  const ctcn_fbank_opts f = mfcc_fbank_opts(opts);
  return fbank_launch("ctcn_mfcc", KIND_MFCC, &f, g.fb, g.nceps, g.fb.nbins * g.nceps + g.nceps, wave, wave_is_int16, lens, plan, mean, scale, feats, frames,
                      B, Nmax, Tmax, dither, seed, utt_offset, stream);
}

extern "C" size_t ctcn_cmvn_accumulate_ws_bytes(int B, int Tmax, int F) {
  if (B <= 0 || Tmax <= 0 || F <= 0) return 0;
  return (size_t)B * ceil_div(Tmax, CMVN_ROWS) * 2 * F * sizeof(double);
}

extern "C" int ctcn_cmvn_accumulate(const float *feats, const int32_t *frames, double *stats, int B, int Tmax, int F, void *ws, size_t ws_bytes,
                                    void *stream) {
  CTCN_REQUIRE(feats && frames && stats && B > 0 && Tmax > 0 && F > 0 && B <= 65535, "ctcn_cmvn_accumulate: bad args");
  const size_t need = ctcn_cmvn_accumulate_ws_bytes(B, Tmax, F);
  CTCN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)stats & 7) == 0, "ctcn_cmvn_accumulate: workspace of ctcn_cmvn_accumulate_ws_bytes needed, 8-byte aligned");
  if (ws_bytes < need) { ctcn_set_error("ctcn_cmvn_accumulate: workspace %zu < %zu bytes", ws_bytes, need); return CTCN_EWORKSPACE; }
  const int chunks = ceil_div(Tmax, CMVN_ROWS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cmvn_partial_kernel, dim3(chunks, B), dim3(256), 0, st, feats, frames, static_cast<double *>(ws), Tmax, F);
  CTCN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cmvn_finish_kernel, dim3(ceil_div(2 * F + 1, 256)), dim3(256), 0, st, static_cast<const double *>(ws), frames, stats, B, Tmax, F, chunks);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_cmvn_accumulate_groups(const float *feats, const int32_t *frames, const int32_t *group, double *stats, int B, int Tmax, int F,
                                           int G, void *ws, size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(feats && frames && group && stats && B > 0 && Tmax > 0 && F > 0 && B <= 65535 && G > 0 && G <= 65535,
               "ctcn_cmvn_accumulate_groups: bad args (B %d and G %d at most 65 535)", B, G);
  const size_t need = ctcn_cmvn_accumulate_ws_bytes(B, Tmax, F);
  CTCN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)stats & 7) == 0,
               "ctcn_cmvn_accumulate_groups: workspace of ctcn_cmvn_accumulate_ws_bytes needed, 8-byte aligned");
  if (ws_bytes < need) { ctcn_set_error("ctcn_cmvn_accumulate_groups: workspace %zu < %zu bytes", ws_bytes, need); return CTCN_EWORKSPACE; }
  const int chunks = ceil_div(Tmax, CMVN_ROWS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cmvn_partial_kernel, dim3(chunks, B), dim3(256), 0, st, feats, frames, static_cast<double *>(ws), Tmax, F);
  CTCN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cmvn_finish_groups_kernel, dim3(ceil_div(2 * F + 1, 256), G), dim3(256), 0, st, static_cast<const double *>(ws), frames, group,
                     stats, B, Tmax, F, chunks);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" size_t ctcn_spectrogram_plan_bytes(const ctcn_spectrogram_opts *opts) {
  FbankGeom g;
  const char *why;
  return spectrogram_geom(opts, &g, &why) == CTCN_OK ? g.words * 4 : 0;
}

extern "C" int ctcn_spectrogram_plan(const ctcn_spectrogram_opts *opts, void *plan, size_t plan_bytes) {
  FbankGeom g;
  const char *why;
  const int rc = spectrogram_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_spectrogram_plan: %s", why); return rc; }
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4, "ctcn_spectrogram_plan: buffer of %zu bytes needed", g.words * 4);
  const ctcn_fbank_opts f = spectrogram_fbank_opts(opts);
  fbank_build_window(&f, g, plan);
  return CTCN_OK;
}

extern "C" int ctcn_spectrogram(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_spectrogram_opts *opts, const void *plan,
                                const float *mean, const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither,
                                uint64_t seed, uint64_t utt_offset, void *stream) {
  FbankGeom g;
  const char *why;
  const int rc = spectrogram_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_spectrogram: %s", why); return rc; }
  const ctcn_fbank_opts f = spectrogram_fbank_opts(opts);
  return fbank_launch("ctcn_spectrogram", KIND_SPEC, &f, g, g.F, 0, wave, wave_is_int16, lens, plan, mean, scale, feats, frames, B, Nmax, Tmax, dither,
                      seed, utt_offset, stream);
}

extern "C" int ctcn_logspec_frames(long long num_samples, int hop) {
  CTCN_REQUIRE(num_samples >= 0 && hop > 0, "ctcn_logspec_frames: bad args (samples %lld, hop %d)", num_samples, hop);
  CTCN_REQUIRE(num_samples / hop < 0x7ffffffeLL, "ctcn_logspec_frames: frame count beyond int");
  return logspec_num_frames(num_samples, hop);
}

extern "C" size_t ctcn_logspec_plan_bytes(const ctcn_logspec_opts *opts) {
  LogSpecGeom g;
  const char *why;
  return logspec_geom(opts, &g, &why) == CTCN_OK ? g.words * 4 : 0;
}

extern "C" int ctcn_logspec_plan(const ctcn_logspec_opts *opts, void *plan, size_t plan_bytes) {
  LogSpecGeom g;
  const char *why;
  const int rc = logspec_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_logspec_plan: %s", why); return rc; }
  CTCN_REQUIRE(plan && plan_bytes >= g.words * 4, "ctcn_logspec_plan: buffer of %zu bytes needed", g.words * 4);
  logspec_build_plan(opts, g, plan);
  return CTCN_OK;
}

// frames per workgroup: eight where the staged samples fit in LDS, else fewer; 0: not even one frame does
static int logspec_fpw(const LogSpecGeom &g) {
  int fpw = 8;
  while (fpw > 1 && logspec_lds_words(g.nfft, g.wpad, g.hop, fpw) * 4 > FBANK_LDS_LIMIT) fpw >>= 1;
  return logspec_lds_words(g.nfft, g.wpad, g.hop, fpw) * 4 > FBANK_LDS_LIMIT ? 0 : fpw;
}

extern "C" size_t ctcn_logspec_ws_bytes(const ctcn_logspec_opts *opts, int B, int Tmax) {
  LogSpecGeom g;
  const char *why;
  if (logspec_geom(opts, &g, &why) != CTCN_OK || B <= 0 || Tmax < 0) return 0;
  const int fpw = logspec_fpw(g);
  return fpw ? (size_t)B * std::max(ceil_div(Tmax, fpw), 1) * 2 * sizeof(double) : 0;
}

extern "C" int ctcn_logspec(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_logspec_opts *opts, const void *plan, float *feats,
                            int32_t *frames, float *stats, int B, int Nmax, int Tmax, void *ws, size_t ws_bytes, void *stream) {
  LogSpecGeom g;
  const char *why;
  const int rc = logspec_geom(opts, &g, &why);
  if (rc != CTCN_OK) { ctcn_set_error("ctcn_logspec: %s", why); return rc; }
  CTCN_REQUIRE(lens && plan && frames && stats && B > 0 && B <= 65535 && Nmax >= 0 && Tmax >= 0 && (wave || Nmax == 0) && (feats || Tmax == 0),
               "ctcn_logspec: bad args (B %d at most 65 535)", B);
  const int fpw = logspec_fpw(g);
  if (!fpw) { ctcn_set_error("ctcn_logspec: window stride of %d samples too long for the LDS staging", g.hop); return CTCN_EUNSUPPORTED; }
  const size_t need = ctcn_logspec_ws_bytes(opts, B, Tmax);
  CTCN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "ctcn_logspec: workspace of ctcn_logspec_ws_bytes needed, 8-byte aligned");
  if (ws_bytes < need) { ctcn_set_error("ctcn_logspec: workspace %zu < %zu bytes", ws_bytes, need); return CTCN_EWORKSPACE; }
  const size_t lds = logspec_lds_words(g.nfft, g.wpad, g.hop, fpw) * 4;
  LogSpecArgs a;
  a.wave = wave; a.lens = lens; a.plan = static_cast<const float *>(plan); a.feats = feats; a.frames = frames; a.stats = stats;
  a.ws = static_cast<double *>(ws);
  a.is_i16 = wave_is_int16 != 0; a.Nmax = Nmax; a.Tmax = Tmax; a.hop = g.hop; a.fpw = fpw; a.normalize = opts->normalize != 0;
  a.in_scale = opts->input_scale;
  const dim3 grid(std::max(ceil_div(Tmax, fpw), 1), B);
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
