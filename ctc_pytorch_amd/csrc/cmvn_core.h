// cmvn_core.h -- the arithmetic of the grouped and the sliding-window mean / variance normalisation, shared by the kernels of cmvn.hip and
// their host twins (ctcn_cmvn_norm_host, ctcn_cmvn_sliding_window, ctcn_cmvn_sliding_host): one definition, so that host and device agree
// bit for bit.  The contract is in include/ctcn.h.  Every float64 operation below is rounded on its own: no function here may be compiled
// into fused multiply-adds, hence the pragma in each of them.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#define CMVN_HD __host__ __device__ inline

// a correctly rounded square root on both sides
CMVN_HD double cmvn_sqrt(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(v);
#else
  return sqrt(v);
#endif
}

// Mean and scale of one column of a statistics matrix: GlobalCMVN.mean_scale's formulas.  n > 0.
CMVN_HD void cmvn_norm(double sum, double sumsq, double n, int norm_vars, float *mean, float *scale) {
#pragma clang fp contract(off)
  const double m = sum / n;
  *mean = (float)m;
  if (!norm_vars) {
    *scale = 1.0f;
    return;
  }
  const double mm = m * m;
  double var = sumsq / n - mm;
  if (var < 1e-20) var = 1e-20;
  *scale = (float)(1.0 / cmvn_sqrt(var));
}

// the feature kernels' expression: a float32 subtraction, then a float32 multiplication
CMVN_HD float cmvn_apply_one(float x, float mean, float scale) {
#pragma clang fp contract(off)
  const float d = x - mean;
  return d * scale;
}

// Kaldi's SlidingWindowCmn window of frame t in an utterance of n frames: [*s, *e).  0 <= t < n, 1 <= min_window <= window.
CMVN_HD void cmvn_window(int t, int n, int window, int min_window, int center, int *s, int *e) {
  int ws, we;
  if (center) {
    ws = t - window / 2;
    we = ws + window;
  } else {
    ws = t - window;
    we = t + 1;
  }
  if (ws < 0) {
    we -= ws;
    ws = 0;
  }
  if (!center && we > t) we = (t + 1 > min_window) ? t + 1 : min_window;
  if (we > n) {
    ws -= we - n;
    we = n;
    if (ws < 0) ws = 0;
  }
  *s = ws;
  *e = we;
}

// the running sums: one frame leaves, one frame enters
CMVN_HD void cmvn_slide_sub(double *S, double *Q, float x) {
#pragma clang fp contract(off)
  const double v = (double)x, vv = v * v;
  *S = *S - v;
  *Q = *Q - vv;
}
CMVN_HD void cmvn_slide_add(double *S, double *Q, float x) {
#pragma clang fp contract(off)
  const double v = (double)x, vv = v * v;
  *S = *S + v;
  *Q = *Q + vv;
}

// the output of frame t from the sums over its window of w frames.  A window of one frame has variance 1: the factor becomes 1.0 by a select
// behind the arithmetic (d * 1.0 is d), so the kernel's chain of frames stays free of branches.
CMVN_HD float cmvn_slide_out(float x, double S, double Q, int w, int norm_vars) {
#pragma clang fp contract(off)
  const double dw = (double)w;
  const double m = S / dw;
  const double d = (double)x - m;
  if (!norm_vars) return (float)d;
  const double mm = m * m;
  double v = Q / dw - mm;
  if (v < 1e-10) v = 1e-10;
  double inv = 1.0 / cmvn_sqrt(v);
  if (w <= 1) inv = 1.0;
  return (float)(d * inv);
}
