// fbank_core.h -- the parts of the filterbank front-end (fbank.hip) that are plain arithmetic on the options or on one frame: the geometry of a
// configuration, the host-side plan builder (filterbank, and the MFCC's DCT table and lifter behind it), the layout of a workgroup's LDS (what
// the kernels read through and their launches size) and the FFT butterflies.  Everything here compiles for the host too, so the plan builders and the
// FFT passes can be exercised by a stand-alone host program (one loop over the 64 "lanes" per pass stands in for the wave).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ctcn.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define FB_HD __host__ __device__ inline

// The FFT runs in float64: a float32 transform leaves noise of ~1e-7 of the frame's RMS in EVERY bin, which the log turns into 1e-4 .. 1e-3 on
// the weakest mel filters (pre-emphasis leaves the lowest ones 1e-4 of the spectrum's amplitude); in float64 the features carry the float32
// rounding of the steps in front of the transform and behind it only.
struct fbc { double x, y; };

constexpr int FBANK_MAX_BINS = 128;

// Word offsets of the plan block (layout in include/ctcn.h) and what the kernel needs to know of a configuration.
struct FbankGeom {
  int L, shift, npad, nbins, F;
  int off_win, off_tw, off_first, off_count, off_woff, off_wts;
  size_t words;
};

FB_HD int fbank_num_frames(long long n, int L, int shift, int snip) {
  if (snip) return n < L ? 0 : (int)(1 + (n - L) / shift);
  return (int)((n + shift / 2) / shift);
}

// CTCN_OK and *g, or the error code with *why pointing at a literal.  mel == false (the spectrogram): no mel bank, so num_mel_bins is not
// looked at, the row is the Npad / 2 + 1 bins and the plan ends behind the twiddles.
inline int fbank_geom(const ctcn_fbank_opts *o, FbankGeom *g, const char **why, bool mel = true) {
  *why = "";
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (!(o->samp_freq > 0.f) || !(o->frame_length_ms > 0.f) || !(o->frame_shift_ms > 0.f)) { *why = "sample rate, frame length and frame shift must be positive"; return CTCN_EINVAL; }
  const double len = (double)o->samp_freq * 0.001 * (double)o->frame_length_ms, sh = (double)o->samp_freq * 0.001 * (double)o->frame_shift_ms;
  if (len >= 1e6 || sh >= 1e6) { *why = "frame length or shift beyond 1e6 samples"; return CTCN_EUNSUPPORTED; }
  g->L = (int)len;                                   // Kaldi: static_cast<int32>(samp_freq * 0.001 * frame_length_ms)
  g->shift = (int)sh;
  if (g->L < 2 || g->shift < 1) { *why = "frame length below 2 samples or frame shift below 1"; return CTCN_EINVAL; }
  if (o->window_type < 0 || o->window_type > 4) { *why = "unknown window type"; return CTCN_EINVAL; }
  if (!(o->preemph_coeff >= 0.f && o->preemph_coeff <= 1.f)) { *why = "preemphasis coefficient outside [0, 1]"; return CTCN_EINVAL; }
  if (mel && o->num_mel_bins < 3) { *why = "fewer than 3 mel bins"; return CTCN_EINVAL; }
  if (!o->round_to_power_of_two) { *why = "round_to_power_of_two=false is not supported"; return CTCN_EUNSUPPORTED; }
  if (mel && o->num_mel_bins > FBANK_MAX_BINS) { *why = "more than 128 mel bins are not supported"; return CTCN_EUNSUPPORTED; }
  int npad = 1;
  while (npad < g->L) npad <<= 1;
  if (npad != 256 && npad != 512 && npad != 1024) { *why = "padded frame length must be 256, 512 or 1024"; return CTCN_EUNSUPPORTED; }
  g->npad = npad;
  g->nbins = mel ? o->num_mel_bins : 0;
  g->F = mel ? g->nbins + (o->use_energy ? 1 : 0) : npad / 2 + 1;
  g->off_win = 0;
  g->off_tw = npad;
  g->off_first = 5 * npad;
  g->off_count = g->off_first + FBANK_MAX_BINS;
  g->off_woff = g->off_count + FBANK_MAX_BINS;
  g->off_wts = g->off_woff + FBANK_MAX_BINS;
  g->words = mel ? (size_t)g->off_wts + npad : (size_t)g->off_first;
  return CTCN_OK;
}

inline double fbank_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

// Words [0, 5 Npad) of the plan: the window of feature-window.cc and the twiddles.
inline void fbank_build_window(const ctcn_fbank_opts *o, const FbankGeom &g, void *plan) {
  const double two_pi = 6.283185307179586476925286766559;
  float *w = (float *)plan;
  memset(plan, 0, g.words * 4);
  const double a = two_pi / (g.L - 1);
  for (int i = 0; i < g.L; ++i) {
    const double x = (double)i;
    double v;
    switch (o->window_type) {
      case 0: v = 0.54 - 0.46 * cos(a * x); break;
      case 1: v = 0.5 - 0.5 * cos(a * x); break;
      case 2: v = pow(0.5 - 0.5 * cos(a * x), 0.85); break;
      case 3: v = 1.0; break;
      default: v = (double)o->blackman_coeff - 0.5 * cos(a * x) + (0.5 - (double)o->blackman_coeff) * cos(2 * a * x); break;
    }
    w[g.off_win + i] = (float)v;
  }
  double *tw = (double *)(w + g.off_tw);                // 8-byte aligned: the block is, and off_tw = npad words
  for (int k = 0; k < g.npad; ++k) {
    tw[2 * k] = cos(two_pi * k / g.npad);
    tw[2 * k + 1] = -sin(two_pi * k / g.npad);
  }
}

// Fills `plan` (g.words 4-byte words).  Window: feature-window.cc; bank: mel-computations.cc without VTLN.
inline int fbank_build_plan(const ctcn_fbank_opts *o, const FbankGeom &g, void *plan, const char **why) {
  float *w = (float *)plan;
  int32_t *iw = (int32_t *)plan;
  fbank_build_window(o, g, plan);
  const double sf = (double)o->samp_freq, nyquist = 0.5 * sf, low = (double)o->low_freq;
  const double high = o->high_freq > 0.f ? (double)o->high_freq : nyquist + (double)o->high_freq;
  if (low < 0.0 || low >= nyquist || high <= 0.0 || high > nyquist || high <= low) { *why = "low_freq / high_freq outside [0, Nyquist] or not in order"; return CTCN_EINVAL; }
  const int nfft = g.npad / 2;
  const double bin_width = sf / g.npad, mel_low = fbank_mel(low), mel_high = fbank_mel(high);
  const double delta = (mel_high - mel_low) / (g.nbins + 1);
  int used = 0;
  for (int b = 0; b < g.nbins; ++b) {
    const double left = mel_low + b * delta, center = mel_low + (b + 1) * delta, right = mel_low + (b + 2) * delta;
    int first = -1, last = -1;
    for (int i = 0; i < nfft; ++i) {
      const double mel = fbank_mel(bin_width * i);
      if (mel > left && mel < right) {
        const double wt = mel <= center ? (mel - left) / (center - left) : (right - mel) / (right - center);
        if (first < 0) first = i;
        last = i;
        if (used >= g.npad) { *why = "mel bank larger than the plan"; return CTCN_EINVAL; }
        w[g.off_wts + used++] = (float)wt;
      }
    }
    if (first < 0) { *why = "a mel filter holds no FFT bin (num_mel_bins too large)"; return CTCN_EINVAL; }
    iw[g.off_first + b] = first;
    iw[g.off_count + b] = last - first + 1;
    iw[g.off_woff + b] = used - (last - first + 1);
    if (o->htk_compat && b == 0 && low != 0.0) w[g.off_wts + iw[g.off_woff + b]] = 0.f;    // HTK's first-bin quirk, as Kaldi's htk_mode replicates it
  }
  return CTCN_OK;
}

// ---- MFCC: the filterbank plan of the same frame and mel options, then the DCT table and the lifter ------------------------------------------------
constexpr int MFCC_MAX_CEPS = 64;                      // one lane per coefficient; a 128 x 64 table is 32 KB of LDS

struct MfccGeom {
  FbankGeom fb;                                        // fb.F is the filterbank's; the MFCC row has nceps columns
  int nceps, off_dct, off_lift;
  size_t words;
};

// The filterbank options an MFCC configuration runs stages 1-4 with: log of the mel-filtered power spectrum, always.
inline ctcn_fbank_opts mfcc_fbank_opts(const ctcn_mfcc_opts *o) {
  ctcn_fbank_opts f;
  memset(&f, 0, sizeof f);
  f.samp_freq = o->samp_freq; f.frame_shift_ms = o->frame_shift_ms; f.frame_length_ms = o->frame_length_ms; f.preemph_coeff = o->preemph_coeff;
  f.blackman_coeff = o->blackman_coeff; f.low_freq = o->low_freq; f.high_freq = o->high_freq; f.energy_floor = o->energy_floor;
  f.window_type = o->window_type; f.num_mel_bins = o->num_mel_bins; f.remove_dc_offset = o->remove_dc_offset;
  f.round_to_power_of_two = o->round_to_power_of_two; f.snip_edges = o->snip_edges; f.use_energy = o->use_energy; f.raw_energy = o->raw_energy;
  f.htk_compat = o->htk_compat; f.use_log_fbank = 1; f.use_power = 1;
  return f;
}

// As fbank_geom: every refusal of the filterbank geometry first, then the MFCC's own.
inline int mfcc_geom(const ctcn_mfcc_opts *o, MfccGeom *g, const char **why) {
  *why = "";
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  const ctcn_fbank_opts f = mfcc_fbank_opts(o);
  const int rc = fbank_geom(&f, &g->fb, why);
  if (rc != CTCN_OK) return rc;
  if (o->num_ceps < 1 || o->num_ceps > o->num_mel_bins) { *why = "num_ceps outside [1, num_mel_bins]"; return CTCN_EINVAL; }
  if (!(o->cepstral_lifter >= 0.f)) { *why = "negative cepstral lifter"; return CTCN_EINVAL; }
  if (o->num_ceps > MFCC_MAX_CEPS) { *why = "more than 64 cepstral coefficients are not supported"; return CTCN_EUNSUPPORTED; }
  g->nceps = o->num_ceps;
  g->off_dct = (int)g->fb.words;
  g->off_lift = g->off_dct + g->fb.nbins * g->nceps;
  g->words = (size_t)g->off_lift + g->nceps;
  return CTCN_OK;
}

// Fills `plan` (g.words words): the filterbank block, then the first nceps rows of Kaldi's ComputeDctMatrix stored bin-major (D[n * nceps + k]:
// lanes that own consecutive cepstra read consecutive words), then the lifter 1 + Q/2 sin(pi k / Q) (ones for Q = 0).  Double, rounded once.
inline int mfcc_build_plan(const ctcn_mfcc_opts *o, const MfccGeom &g, void *plan, const char **why) {
  const double pi = 3.14159265358979323846;
  const ctcn_fbank_opts f = mfcc_fbank_opts(o);
  const int rc = fbank_build_plan(&f, g.fb, plan, why);
  if (rc != CTCN_OK) return rc;
  float *w = (float *)plan;
  const int N = g.fb.nbins, C = g.nceps;
  for (int n = 0; n < N; ++n) {
    w[g.off_dct + n * C] = (float)sqrt(1.0 / N);
    for (int k = 1; k < C; ++k) w[g.off_dct + n * C + k] = (float)(sqrt(2.0 / N) * cos(pi / N * (n + 0.5) * k));
  }
  const double Q = (double)o->cepstral_lifter;
  for (int k = 0; k < C; ++k) w[g.off_lift + k] = Q != 0.0 ? (float)(1.0 + 0.5 * Q * sin(pi * k / Q)) : 1.f;
  return CTCN_OK;
}

// ---- Kaldi's spectrogram: stages 1-3 of the filterbank, no mel bank --------------------------------------------------------------------------
// The filterbank options a spectrogram configuration runs stages 1-3 with: the energy always, in column 0.
inline ctcn_fbank_opts spectrogram_fbank_opts(const ctcn_spectrogram_opts *o) {
  ctcn_fbank_opts f;
  memset(&f, 0, sizeof f);
  f.samp_freq = o->samp_freq; f.frame_shift_ms = o->frame_shift_ms; f.frame_length_ms = o->frame_length_ms; f.preemph_coeff = o->preemph_coeff;
  f.blackman_coeff = o->blackman_coeff; f.energy_floor = o->energy_floor; f.window_type = o->window_type;
  f.remove_dc_offset = o->remove_dc_offset; f.round_to_power_of_two = o->round_to_power_of_two; f.snip_edges = o->snip_edges;
  f.use_energy = 1; f.raw_energy = o->raw_energy; f.use_log_fbank = 1; f.use_power = 1;
  return f;
}

// As fbank_geom without the mel bank's refusals; return_raw_fft is Kaldi's option and not built.
inline int spectrogram_geom(const ctcn_spectrogram_opts *o, FbankGeom *g, const char **why) {
  *why = "";
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  const ctcn_fbank_opts f = spectrogram_fbank_opts(o);
  const int rc = fbank_geom(&f, g, why, false);
  if (rc != CTCN_OK) return rc;
  if (o->return_raw_fft) { *why = "return_raw_fft=true is not supported"; return CTCN_EUNSUPPORTED; }
  return CTCN_OK;
}

// ---- the recipe's log-magnitude STFT (ctcn_logspec) ------------------------------------------------------------------------------------------
struct LogSpecGeom {
  int nfft, hop, wpad, F;                              // wpad: the window's entries, nfft rounded up to a multiple of 64
  int off_win, off_tw;
  size_t words;
};

FB_HD int logspec_num_frames(long long n, int hop) { return n <= 0 ? 0 : (int)(1 + n / hop); }

// Index i (any sign) of a signal of n >= 1 samples extended as numpy.pad(mode="reflect") does: the edge sample is not repeated, period 2 (n - 1)
FB_HD long long logspec_reflect(long long i, long long n) {
  if (n == 1) return 0;
  const long long p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

inline int logspec_geom(const ctcn_logspec_opts *o, LogSpecGeom *g, const char **why) {
  *why = "";
  if (!o) { *why = "null options"; return CTCN_EINVAL; }
  if (!(o->sample_rate > 0.0) || !(o->window_size > 0.0) || !(o->window_stride > 0.0)) { *why = "sample rate, window size and window stride must be positive"; return CTCN_EINVAL; }
  if (o->window < 0 || o->window > 3) { *why = "unknown window"; return CTCN_EINVAL; }
  if (!(o->input_scale > 0.f) || !(o->input_scale < INFINITY)) { *why = "input scale must be positive and finite"; return CTCN_EINVAL; }
  const double len = o->sample_rate * o->window_size, sh = o->sample_rate * o->window_stride;
  if (len >= 1e6 || sh >= 1e6) { *why = "window size or stride beyond 1e6 samples"; return CTCN_EUNSUPPORTED; }
  g->nfft = (int)len;                                  // the reference: int(sample_rate * window_size), in double
  g->hop = (int)sh;
  if (g->hop < 1) { *why = "window stride below 1 sample"; return CTCN_EINVAL; }
  if (g->nfft != 256 && g->nfft != 400 && g->nfft != 512 && g->nfft != 1024) { *why = "n_fft must be 256, 400, 512 or 1024"; return CTCN_EUNSUPPORTED; }
  g->wpad = (g->nfft + 63) / 64 * 64;
  g->F = g->nfft / 2 + 1;
  g->off_win = 0;
  g->off_tw = 2 * g->wpad;
  g->words = (size_t)g->off_tw + 4 * (size_t)g->nfft;
  return CTCN_OK;
}

// Fills `plan` (g.words words): scipy.signal.windows' symmetric forms in double (kept in double: a float32 window, or a float32 product with
// it, leaves ~1e-3 of absolute noise in every bin, 1e-5 of the log1p in a valley 500 times below the spectrum's level), zeros behind n_fft;
// then the twiddles.
inline void logspec_build_plan(const ctcn_logspec_opts *o, const LogSpecGeom &g, void *plan) {
  const double two_pi = 6.283185307179586476925286766559;
  double *w = (double *)plan;
  memset(plan, 0, g.words * 4);
  const int N = g.nfft;
  const double a = two_pi / (N - 1);
  for (int i = 0; i < N; ++i) {
    double v;
    switch (o->window) {
      case 0: v = 0.54 - 0.46 * cos(a * i); break;
      case 1: v = 0.5 - 0.5 * cos(a * i); break;
      case 2: v = 0.42 - 0.5 * cos(a * i) + 0.08 * cos(2 * a * i); break;
      default: v = 2 * i <= N - 1 ? 2.0 * i / (N - 1) : 2.0 - 2.0 * i / (N - 1); break;
    }
    w[i] = v;
  }
  double *tw = (double *)plan + g.off_tw / 2;
  for (int k = 0; k < N; ++k) {
    tw[2 * k] = cos(two_pi * k / N);
    tw[2 * k + 1] = -sin(two_pi * k / N);
  }
}

// ---- the LDS of a workgroup ---------------------------------------------------------------------------------------------------------------
// The head of each kernel's dynamic LDS is a struct: the kernel reads its regions as members and the launch sizes the allocation and the
// frames per workgroup from its sizeof, so the two cannot drift apart.  Behind the head lie fbank_lds_table words, then lds_samples words.
// (tests/test_spectrogram_host.py compiles this header and holds every offset and size to the kernels' earlier pointer arithmetic.)
enum { KIND_FBANK = 0, KIND_MFCC = 1, KIND_SPEC = 2 };                 // the feature types of fbank_kernel

template <int NPAD>
struct FbankLds {
  fbc tw[NPAD];                                        // twiddles
  double wbuf[4][2][NPAD];                             // 4 waves x 2 buffers of NPAD / 2 complex
  float win[NPAD];                                     // the window, 0 from L on
  float wts[NPAD];                                     // the filters' weights, back to back
  int ftab[3 * FBANK_MAX_BINS];                        // first | count | weight offset, FBANK_MAX_BINS each
};

template <int N>
struct LogSpecLds {
  fbc tw[N];                                           // twiddles
  double wbuf[4][2][N];                                // 4 waves x 2 buffers of N / 2 complex
  double red[8];                                       // 4 waves x (sum, sum of squares)
  double win[(N + 63) / 64 * 64];                      // the float64 window, zeros behind N
};

// bytes of the head for a length known at run time (the lengths fbank_geom / logspec_geom admit)
constexpr size_t fbank_lds_head(int npad) { return npad == 256 ? sizeof(FbankLds<256>) : npad == 512 ? sizeof(FbankLds<512>) : sizeof(FbankLds<1024>); }
constexpr size_t logspec_lds_head(int n) { return n == 256 ? sizeof(LogSpecLds<256>) : n == 400 ? sizeof(LogSpecLds<400>) : n == 512 ? sizeof(LogSpecLds<512>) : sizeof(LogSpecLds<1024>); }
FB_HD constexpr int fbank_lds_table(int nbins, int F, int kind) { return kind == KIND_MFCC ? nbins * F + F : 0; }      // DCT, nbins x F bin-major, then the lifter (F)
FB_HD constexpr size_t lds_samples(int fpw, int shift, int L) { return (size_t)(fpw - 1) * shift + L; }                 // of fpw neighbouring frames

// ---- FFT butterflies: forward DFTs of 2, 4 and 8 points, natural order in and out -------------------------------------------------------------
FB_HD fbc fb_c(double x, double y) { fbc r; r.x = x; r.y = y; return r; }
FB_HD fbc fb_add(fbc a, fbc b) { return fb_c(a.x + b.x, a.y + b.y); }
FB_HD fbc fb_sub(fbc a, fbc b) { return fb_c(a.x - b.x, a.y - b.y); }
FB_HD fbc fb_mul(fbc a, fbc b) { return fb_c(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
FB_HD fbc fb_mul_mi(fbc a) { return fb_c(a.y, -a.x); }      // a * (-i)

template <int R> struct FbDft;
template <> struct FbDft<2> {
  FB_HD static void run(fbc *v) {
    const fbc a = v[0], b = v[1];
    v[0] = fb_add(a, b);
    v[1] = fb_sub(a, b);
  }
};
template <> struct FbDft<4> {
  FB_HD static void run(fbc *v) {
    const fbc s02 = fb_add(v[0], v[2]), d02 = fb_sub(v[0], v[2]), s13 = fb_add(v[1], v[3]), d13 = fb_mul_mi(fb_sub(v[1], v[3]));
    v[0] = fb_add(s02, s13);
    v[1] = fb_add(d02, d13);
    v[2] = fb_sub(s02, s13);
    v[3] = fb_sub(d02, d13);
  }
};
template <> struct FbDft<8> {
  FB_HD static void run(fbc *v) {
    const double h = 0.70710678118654752440;
    fbc e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
    FbDft<4>::run(e);
    FbDft<4>::run(o);
    o[1] = fb_c(h * (o[1].x + o[1].y), h * (o[1].y - o[1].x));       // * (1 - i) / sqrt 2
    o[2] = fb_mul_mi(o[2]);
    o[3] = fb_c(h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y));      // * (-1 - i) / sqrt 2
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = fb_add(e[k], o[k]);
      v[k + 4] = fb_sub(e[k], o[k]);
    }
  }
};

template <> struct FbDft<5> {
  FB_HD static void run(fbc *v) {
    const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;   // cos(2 pi / 5), cos(4 pi / 5)
    const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;    // sin(2 pi / 5), sin(4 pi / 5)
    const fbc a = v[0], p1 = fb_add(v[1], v[4]), m1 = fb_sub(v[1], v[4]), p2 = fb_add(v[2], v[3]), m2 = fb_sub(v[2], v[3]);
    const fbc e1 = fb_c(a.x + c1 * p1.x + c2 * p2.x, a.y + c1 * p1.y + c2 * p2.y);
    const fbc e2 = fb_c(a.x + c2 * p1.x + c1 * p2.x, a.y + c2 * p1.y + c1 * p2.y);
    const fbc o1 = fb_c(s1 * m1.y + s2 * m2.y, -(s1 * m1.x + s2 * m2.x));     // -i (s1 m1 + s2 m2)
    const fbc o2 = fb_c(s2 * m1.y - s1 * m2.y, -(s2 * m1.x - s1 * m2.x));     // -i (s2 m1 - s1 m2)
    v[0] = fb_c(a.x + p1.x + p2.x, a.y + p1.y + p2.y);
    v[1] = fb_add(e1, o1);
    v[2] = fb_add(e2, o2);
    v[3] = fb_sub(e2, o2);
    v[4] = fb_sub(e1, o1);
  }
};

// The passes of the N / 2-point complex transform behind an N-point real one: three radices whose product is N / 2 (another length is one
// line here, one instantiation in fbank.hip and one case in each of the switches and ladders over the length).
template <int N> struct FbRadix;
template <> struct FbRadix<256> { static constexpr int r0 = 8, r1 = 8, r2 = 2; };
template <> struct FbRadix<400> { static constexpr int r0 = 8, r1 = 5, r2 = 5; };
template <> struct FbRadix<512> { static constexpr int r0 = 8, r1 = 8, r2 = 4; };
template <> struct FbRadix<1024> { static constexpr int r0 = 8, r1 = 8, r2 = 8; };

// One Stockham (autosort) pass of radix R over M complex points, Ns = the product of the radices of the passes before it (R Ns divides M; M
// and Ns need not be powers of two): lane `lane` of 64 takes butterflies lane, lane + 64, ...  tw[k] = exp(-2 pi i k / (2 M)), k < 2 M.  in
// and out are different buffers.
template <int M, int R>
FB_HD void fbank_fft_pass(int lane, int Ns, const fbc *in, fbc *out, const fbc *tw) {
  for (int j = lane; j < M / R; j += 64) {
    fbc v[R];
    const int k = (int)((unsigned)j % (unsigned)Ns);  // (an AND where Ns is a power of two: every call passes a constant)
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = in[j + r * (M / R)];
    if (Ns > 1) {
      const int step = 2 * k * (M / (Ns * R));        // k r / (Ns R) of a turn = table index r * step < 2 M
#pragma unroll
      for (int r = 1; r < R; ++r) v[r] = fb_mul(v[r], tw[r * step]);
    }
    FbDft<R>::run(v);
    const int d = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) out[d + r * Ns] = v[r];
  }
}

// Bin k of the real transform of x[0 .. 2M) from Z = the M-point transform of z[m] = x[2m] + i x[2m+1]: |X[k]|^2, k < M.
template <int M>
FB_HD double fbank_split_power(int k, const fbc *Z, const fbc *tw) {
  const fbc a = Z[k], b = Z[k ? M - k : 0];
  const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);      // (Z[k] + conj Z[M-k]) / 2
  const double odr = 0.5 * (a.y + b.y), odi = -0.5 * (a.x - b.x);   // (Z[k] - conj Z[M-k]) / 2i
  const fbc t = fb_mul(fb_c(odr, odi), tw[k]);
  const double xr = er + t.x, xi = ei + t.y;
  return xr * xr + xi * xi;
}

// Bin M, the Nyquist bin the split step's loop does not reach: X[M] = Re Z[0] - Im Z[0], real.
FB_HD double fbank_nyquist_power(const fbc *Z) {
  const double d = Z[0].x - Z[0].y;
  return d * d;
}

// The N-point real transform of one frame on the host, by the passes and the split step above with a loop over the 64 lanes standing in for
// the wave: power[0 .. N/2] = |X[k]|^2.  a, b: N / 2 complex each, a holding the frame as pairs on entry; tw: (cos, -sin)(2 pi k / N), k < N.
template <int N>
inline void fbank_power_host(fbc *a, fbc *b, const fbc *tw, double *power) {
  constexpr int M = N / 2;
  using R = FbRadix<N>;
  static_assert(R::r0 * R::r1 * R::r2 == M, "the radices of a length multiply to half of it");
  for (int lane = 0; lane < 64; ++lane) fbank_fft_pass<M, R::r0>(lane, 1, a, b, tw);
  for (int lane = 0; lane < 64; ++lane) fbank_fft_pass<M, R::r1>(lane, R::r0, b, a, tw);
  for (int lane = 0; lane < 64; ++lane) fbank_fft_pass<M, R::r2>(lane, R::r0 * R::r1, a, b, tw);
  for (int lane = 0; lane < 64; ++lane)
    for (int k = lane; k < M; k += 64) power[k] = fbank_split_power<M>(k, b, tw);
  power[M] = fbank_nyquist_power(b);
}
