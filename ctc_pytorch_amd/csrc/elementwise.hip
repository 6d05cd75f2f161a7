// elementwise.hip -- dropout (Philox), Adam, small reductions and the CNN<->RNN layout shuffles (gfx950).
//
// replaces: nn.Dropout (reference timit/models/model_ctc.py:26,34,58,67), torch.optim.Adam.step
// (timit/steps/train_ctc.py:145,65), and the transpose/view/transpose sequence of CTC_Model.forward
// (model_ctc.py:153-158).  All HBM-bound streaming kernels: 16 B per lane, grid-stride, no LDS.
#include <algorithm>

#include "common.h"

namespace {

// (Philox4x32-10: philox4 in common.h, shared with the fused dropout store of rnn_fwd_tagged)
// y[i] = keep(i) ? x[i]/(1-p) : 0, keep(i) <=> u(i) >= p, u = 24-bit uniform of Philox word (i&3) of group (offset+i)>>2
__global__ void dropout_kernel(const float *__restrict__ x, float *__restrict__ y, size_t n, float p, float scale,
                               uint64_t seed, uint64_t offset) {
  const size_t ngroups = (n + 3) / 4;
  for (size_t gi = blockIdx.x * (size_t)blockDim.x + threadIdx.x; gi < ngroups; gi += (size_t)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4(seed, offset + gi, r);
    const size_t i0 = gi * 4;
    if (i0 + 3 < n && (((uintptr_t)(x + i0) | (uintptr_t)(y + i0)) & 15) == 0) {
      const float4 v = *reinterpret_cast<const float4 *>(x + i0);
      float4 o;
      o.x = ((r[0] >> 8) * (1.0f / 16777216.0f) >= p) ? v.x * scale : 0.0f;
      o.y = ((r[1] >> 8) * (1.0f / 16777216.0f) >= p) ? v.y * scale : 0.0f;
      o.z = ((r[2] >> 8) * (1.0f / 16777216.0f) >= p) ? v.z * scale : 0.0f;
      o.w = ((r[3] >> 8) * (1.0f / 16777216.0f) >= p) ? v.w * scale : 0.0f;
      *reinterpret_cast<float4 *>(y + i0) = o;
    } else {
      for (int c = 0; c < 4 && i0 + c < n; ++c)
        y[i0 + c] = ((r[c] >> 8) * (1.0f / 16777216.0f) >= p) ? x[i0 + c] * scale : 0.0f;
    }
  }
}

// torch.optim.Adam (L2-coupled weight decay), SURVEY Appendix A.9
__global__ void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                            size_t n, float step_size, float beta1, float beta2, float eps, float wd, float sqrt_bc2) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float gv = g[i] + wd * pv;
    const float mv = beta1 * m[i] + (1.0f - beta1) * gv;
    const float vv = beta2 * v[i] + (1.0f - beta2) * gv * gv;
    m[i] = mv; v[i] = vv;
    p[i] = pv - step_size * (mv / (sqrtf(vv) / sqrt_bc2 + eps));
  }
}

__global__ void sum_kernel(const float *__restrict__ x, float *__restrict__ out, int n, const int *__restrict__ status) {
  // single workgroup, fixed order: per-thread strided partials (double) -> wave shuffle -> 4 waves
  __shared__ double s[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)x[i];
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  // the sticky status word of the persistent recurrences (a hand-off timed out in this or an earlier launch): the summed loss
  // becomes NaN, so that a caller that never reads the word -- the reference's own run_epoch -- still sees the failure
  if (threadIdx.x == 0) out[0] = (status && *status != 0) ? __uint_as_float(0x7fc00000u) : (float)(s[0] + s[1] + s[2] + s[3]);
}

// nn.CTCLoss's reduction of the per-utterance losses, nll' = nll with +inf replaced by 0 under zero_infinity:
// 'sum' out[0] = sum_b nll'_b, 'mean' out[0] = (1/B) sum_b nll'_b / max(L_b, 1), 'none' out[b] = nll'_b.  The sums are sum_kernel's: one
// workgroup, the same fixed order and double partials ('sum' without zero_infinity gives its bits), and the same status-word rule.
__global__ void ctc_reduce_kernel(const float *__restrict__ nll, const int64_t *__restrict__ tgt_len, float *__restrict__ out, int B,
                                  int reduction, int zinf, const int *__restrict__ status) {
  __shared__ double s[4];
  const bool failed = status && *status != 0;
  if (reduction == CTCN_REDUCTION_NONE) {
    for (int i = threadIdx.x; i < B; i += 256) {
      const float v = nll[i];
      out[i] = failed ? __uint_as_float(0x7fc00000u) : (zinf && v == INFINITY) ? 0.0f : v;
    }
    return;
  }
  double a = 0.0;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float v = (zinf && nll[i] == INFINITY) ? 0.0f : nll[i];
    if (reduction == CTCN_REDUCTION_MEAN) a += (double)v / (double)(tgt_len[i] > 1 ? tgt_len[i] : 1);
    else a += (double)v;
  }
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = s[0] + s[1] + s[2] + s[3];
    out[0] = failed ? __uint_as_float(0x7fc00000u) : (float)(reduction == CTCN_REDUCTION_MEAN ? t / B : t);
  }
}

// (B,C,T,F) -> (T,B,C*F): out[((t*B+b)*C + c)*F + f] = in[((b*C+c)*T + t)*F + f]
__global__ void bctf_to_tbcf_kernel(const float *__restrict__ in, float *__restrict__ out, int B, int C, int T, int F, int to_tbcf) {
  const size_t total = (size_t)B * C * T * F;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    // i enumerates the (T,B,C,F) side so that the strided side is the read (to_tbcf) or the write (from)
    const int f = i % F;
    size_t q = i / F;
    const int c = q % C; q /= C;
    const int b = q % B;
    const int t = q / B;
    const size_t j = (((size_t)b * C + c) * T + t) * F + f;
    if (to_tbcf) out[i] = in[j]; else out[j] = in[i];
  }
}

// generic gather-copy: out contiguous [d0][d1][d2][d3], in element (i0,i1,i2,i3) at in[i0*s0+i1*s1+i2*s2+i3*s3]
__global__ void copy_strided4_kernel(const float *__restrict__ in, float *__restrict__ out, int d0, int d1, int d2, int d3,
                                     size_t s0, size_t s1, size_t s2, size_t s3) {
  const size_t total = (size_t)d0 * d1 * d2 * d3;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int i3 = i % d3;
    size_t q = i / d3;
    const int i2 = q % d2; q /= d2;
    const int i1 = q % d1;
    const int i0 = q / d1;
    out[i] = in[i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3];
  }
}

__global__ void relu_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = fmaxf(x[i], 0.0f);
}
__global__ void relu_bwd_kernel(const float *__restrict__ y, const float *__restrict__ dy, float *__restrict__ dx, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dx[i] = y[i] > 0.0f ? dy[i] : 0.0f;
}

}  // namespace

extern "C" int ctcn_copy_strided4(const float *in, float *out, int d0, int d1, int d2, int d3, size_t s0, size_t s1, size_t s2,
                                  size_t s3, void *stream) {
  CTCN_REQUIRE(in && out && d0 > 0 && d1 > 0 && d2 > 0 && d3 > 0, "ctcn_copy_strided4: bad args");
  const size_t total = (size_t)d0 * d1 * d2 * d3;
  const int blocks = (int)std::min((size_t)4096, ceil_div_z(total, 256));
  hipLaunchKernelGGL(copy_strided4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in, out, d0, d1, d2, d3, s0, s1, s2, s3);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
extern "C" int ctcn_relu_fwd(const float *x, float *y, size_t n, void *stream) {
  CTCN_REQUIRE(x && y, "ctcn_relu_fwd: null pointer");
  if (n == 0) return CTCN_OK;
  hipLaunchKernelGGL(relu_fwd_kernel, dim3((int)std::min((size_t)4096, ceil_div_z(n, 256))), dim3(256), 0, (hipStream_t)stream, x, y, n);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
extern "C" int ctcn_relu_bwd(const float *y, const float *dy, float *dx, size_t n, void *stream) {
  CTCN_REQUIRE(y && dy && dx, "ctcn_relu_bwd: null pointer");
  if (n == 0) return CTCN_OK;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3((int)std::min((size_t)4096, ceil_div_z(n, 256))), dim3(256), 0, (hipStream_t)stream, y, dy, dx, n);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_dropout(const float *x, float *y, size_t n, float p, uint64_t seed, uint64_t offset, void *stream) {
  CTCN_REQUIRE(x && y, "ctcn_dropout: null pointer");
  CTCN_REQUIRE(p >= 0.0f && p < 1.0f, "ctcn_dropout: p=%f outside [0,1)", (double)p);
  if (n == 0) return CTCN_OK;
  const size_t ng = (n + 3) / 4;
  const int blocks = (int)std::min((size_t)4096, ceil_div_z(ng, 256));
  hipLaunchKernelGGL(dropout_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, n, p, 1.0f / (1.0f - p), seed, offset);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_adam_step(float *p, const float *g, float *m, float *v, size_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int step, void *stream) {
  CTCN_REQUIRE(p && g && m && v && step >= 1, "ctcn_adam_step: bad args");
  if (n == 0) return CTCN_OK;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const int blocks = (int)std::min((size_t)4096, ceil_div_z(n, 256));
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)((double)lr / bc1), beta1,
                     beta2, eps, weight_decay, (float)sqrt(bc2));
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_sum_f32(const float *x, float *out, int n, void *stream) {
  CTCN_REQUIRE(x && out && n >= 0, "ctcn_sum_f32: bad args");
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, out, n, (const int *)ctcn_status_word());
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_ctc_reduce(const float *nll, const int64_t *tgt_len, float *out, int B, int reduction, int zero_infinity, void *stream) {
  CTCN_REQUIRE(nll && out && B > 0 && (tgt_len || reduction != CTCN_REDUCTION_MEAN), "ctcn_ctc_reduce: bad args");
  CTCN_REQUIRE(reduction == CTCN_REDUCTION_NONE || reduction == CTCN_REDUCTION_MEAN || reduction == CTCN_REDUCTION_SUM,
               "ctcn_ctc_reduce: reduction %d", reduction);
  hipLaunchKernelGGL(ctc_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nll, tgt_len, out, B, reduction, zero_infinity != 0,
                     (const int *)ctcn_status_word());
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_bctf_to_tbcf(const float *in, float *out, int B, int C, int T, int F, void *stream) {
  CTCN_REQUIRE(in && out && B > 0 && C > 0 && T > 0 && F > 0, "ctcn_bctf_to_tbcf: bad args");
  const size_t total = (size_t)B * C * T * F;
  const int blocks = (int)std::min((size_t)4096, ceil_div_z(total, 256));
  hipLaunchKernelGGL(bctf_to_tbcf_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in, out, B, C, T, F, 1);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
extern "C" int ctcn_tbcf_to_bctf(const float *in, float *out, int B, int C, int T, int F, void *stream) {
  CTCN_REQUIRE(in && out && B > 0 && C > 0 && T > 0 && F > 0, "ctcn_tbcf_to_bctf: bad args");
  const size_t total = (size_t)B * C * T * F;
  const int blocks = (int)std::min((size_t)4096, ceil_div_z(total, 256));
  hipLaunchKernelGGL(bctf_to_tbcf_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in, out, B, C, T, F, 0);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
