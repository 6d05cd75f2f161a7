// fbank_core.h -- the parts of the filterbank front-end (fbank.hip) that are plain arithmetic on the options or on one frame: the geometry of a
// configuration, the host-side plan builder (filterbank, and the MFCC's DCT table and lifter behind it) and the FFT butterflies.  Everything here
// compiles for the host too, so the plan builders and the
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

// CTCN_OK and *g, or the error code with *why pointing at a literal.
inline int fbank_geom(const ctcn_fbank_opts *o, FbankGeom *g, const char **why) {
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
  if (o->num_mel_bins < 3) { *why = "fewer than 3 mel bins"; return CTCN_EINVAL; }
  if (!o->round_to_power_of_two) { *why = "round_to_power_of_two=false is not supported"; return CTCN_EUNSUPPORTED; }
  if (o->num_mel_bins > FBANK_MAX_BINS) { *why = "more than 128 mel bins are not supported"; return CTCN_EUNSUPPORTED; }
  int npad = 1;
  while (npad < g->L) npad <<= 1;
  if (npad != 256 && npad != 512 && npad != 1024) { *why = "padded frame length must be 256, 512 or 1024"; return CTCN_EUNSUPPORTED; }
  g->npad = npad;
  g->nbins = o->num_mel_bins;
  g->F = g->nbins + (o->use_energy ? 1 : 0);
  g->off_win = 0;
  g->off_tw = npad;
  g->off_first = 5 * npad;
  g->off_count = g->off_first + FBANK_MAX_BINS;
  g->off_woff = g->off_count + FBANK_MAX_BINS;
  g->off_wts = g->off_woff + FBANK_MAX_BINS;
  g->words = (size_t)g->off_wts + npad;
  return CTCN_OK;
}

inline double fbank_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

// Fills `plan` (g.words 4-byte words).  Window: feature-window.cc; bank: mel-computations.cc without VTLN.
inline int fbank_build_plan(const ctcn_fbank_opts *o, const FbankGeom &g, void *plan, const char **why) {
  const double two_pi = 6.283185307179586476925286766559;
  float *w = (float *)plan;
  int32_t *iw = (int32_t *)plan;
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

// One Stockham (autosort) pass of radix R over M complex points, Ns = the product of the radices of the passes before it: lane `lane` of 64
// takes butterflies lane, lane + 64, ...  tw[k] = exp(-2 pi i k / (2 M)), k < 2 M.  in and out are different buffers.
template <int M, int R>
FB_HD void fbank_fft_pass(int lane, int Ns, const fbc *in, fbc *out, const fbc *tw) {
  for (int j = lane; j < M / R; j += 64) {
    fbc v[R];
    const int k = j & (Ns - 1);
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
  const fbc a = Z[k], b = Z[(M - k) & (M - 1)];
  const double er = 0.5 * (a.x + b.x), ei = 0.5 * (a.y - b.y);      // (Z[k] + conj Z[M-k]) / 2
  const double odr = 0.5 * (a.y + b.y), odi = -0.5 * (a.x - b.x);   // (Z[k] - conj Z[M-k]) / 2i
  const fbc t = fb_mul(fb_c(odr, odi), tw[k]);
  const double xr = er + t.x, xi = ei + t.y;
  return xr * xr + xi * xi;
}
