// pitch_core.h -- the arithmetic of the pitch extractor (Kaldi's compute-kaldi-pitch-feats and process-kaldi-pitch-feats), shared by the
// kernels of pitch.hip and their host twins (ctcn_pitch_host, ctcn_pitch_process_host): one definition, so that host and device agree bit
// for bit on steps 4 to 7 of the contract in include/ctcn.h.  Every float64 operation below is rounded on its own: no function here may be
// compiled into fused multiply-adds, hence the pragma in each of them.  Division is IEEE's on both sides, the square root is correctly rounded.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#define PITCH_HD __host__ __device__ inline

constexpr int PITCH_VAR_LANES = 256;               // the shape of the variance's partial sums: lane i sums samples i, i + 256, ...

PITCH_HD double pitch_sqrt(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(v);
#else
  return sqrt(v);
#endif
}

// One sample enters a pair of partial sums (the sum and the sum of squares; a float32 squared is exact in double).
PITCH_HD void pitch_var_add(double *S, double *Q, float x) {
#pragma clang fp contract(off)
  const double v = (double)x, vv = v * v;
  *S = *S + v;
  *Q = *Q + vv;
}

// The ballast of an utterance of m > 0 downsampled samples from its sums: (var W)^2 nccf_ballast, var = Q / m - (S / m)^2.
PITCH_HD double pitch_ballast(double S, double Q, int m, int W, double nccf_ballast) {
#pragma clang fp contract(off)
  const double dm = (double)m;
  const double mean = S / dm;
  const double mm = mean * mean;
  const double var = Q / dm - mm;
  const double vw = var * (double)W;
  const double sq = vw * vw;
  return sq * nccf_ballast;
}

// Mean of the first W samples of a frame's window x (W + last samples, zeros behind the utterance) and the energy of those W samples
// with the mean removed; sample order.
PITCH_HD void pitch_frame_mean(const float *x, int W, double *mean, double *e1) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int i = 0; i < W; ++i) s = s + (double)x[i];
  const double m = s / (double)W;
  double e = 0.0;
  for (int i = 0; i < W; ++i) {
    const double v = (double)x[i] - m;
    const double vv = v * v;
    e = e + vv;
  }
  *mean = m;
  *e1 = e;
}

// The two correlations of one integer lag, kept in double.
PITCH_HD void pitch_nccf_lag(const float *x, int W, int lag, double mean, double e1, double ballast, double *nccf_pitch, double *nccf_pov) {
#pragma clang fp contract(off)
  double e2 = 0.0, inner = 0.0;
  for (int i = 0; i < W; ++i) {
    const double a = (double)x[i] - mean, b = (double)x[lag + i] - mean;
    const double bb = b * b, ab = a * b;
    e2 = e2 + bb;
    inner = inner + ab;
  }
  const double prod = e1 * e2;
  const double dp = pitch_sqrt(prod + ballast), dv = pitch_sqrt(prod);
  *nccf_pitch = dp != 0.0 ? inner / dp : 0.0;
  *nccf_pov = dv != 0.0 ? inner / dv : 0.0;
}

// One value of the upsampled row: n taps from row[0] on (element stride `stride`), tap order, rounded to float32 once.
PITCH_HD float pitch_upsample(const double *row, int stride, const float *w, int n) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int j = 0; j < n; ++j) {
    const double p = (double)w[j] * row[(size_t)j * stride];
    acc = acc + p;
  }
  return (float)acc;
}

// The local cost of a state: 1 - n + (soft_min_f0 lag) n.
PITCH_HD double pitch_local(float nccf_pitch, double soft_lag) {
#pragma clang fp contract(off)
  const double n = (double)nccf_pitch;
  const double a = 1.0 - n, b = soft_lag * n;
  return a + b;
}

// ---- post-processing (step 8): float64 throughout, rounded to float32 once by the caller; held to a tolerance, not to bits ----
PITCH_HD double pitch_pov_feature(double n) {
  if (n > 1.0) n = 1.0;
  if (n < -1.0) n = -1.0;
  return pow(1.0001 - n, 0.15) - 1.0;
}

PITCH_HD double pitch_pov(double n) {
  double a = fabs(n);
  if (a > 1.0) a = 1.0;
  const double r = -5.2 + 5.4 * exp(7.5 * (a - 1.0)) + 4.8 * a - 2.0 * exp(-10.0 * a) + 4.2 * exp(20.0 * (a - 1.0));
  return 1.0 / (1.0 + exp(-r));
}
