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

// ---- global gradient norm, clip decision and the clipped / guarded Adam (nn.utils.clip_grad_norm_ + torch.optim.Adam.step) -------------
// The L2 sum is a function of the buffer's bits alone: chunk c covers elements [c*NORM_CHUNK, (c+1)*NORM_CHUNK) whichever workgroup takes
// it; inside a chunk thread t owns the float4 groups t, t+256, ... (a fixed element -> lane map, also on the unaligned path), adds its
// squares as doubles in element order, the 64 lanes combine in wave_sum_d's butterfly and the 4 waves in index order.  Elements past n
// count as +0.0, which changes no sum.  The square of a float is exact in double, so contraction does not matter here.
constexpr int NORM_CHUNK = 16384;      // elements per chunk partial: a compile-time constant, never the grid's or the device's
constexpr int NORM_SEG_SPLIT = 16;     // partials per segment of the optional per-segment norms

__device__ __forceinline__ float nan_max(float a, float b) { return (b != b) ? b : ((a != a) ? a : fmaxf(a, b)); }     // max that keeps NaN, as torch's
__device__ __forceinline__ double nan_max_d(double a, double b) { return (b != b) ? b : ((a != a) ? a : fmax(a, b)); }

// one value per workgroup (256 threads), valid in thread 0: the sum of `a` (wave butterfly, then waves 0..3 in order) or the NaN-keeping max of `mx`
__device__ __forceinline__ double norm_block_reduce(double a, float mx, int inf, double *s) {
  if (inf) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = nan_max(mx, __shfl_xor(mx, o, 64));
    a = (double)mx;
  } else {
    a = wave_sum_d(a);
  }
  __syncthreads();                      // the previous value of s has been read
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  if (inf) return nan_max_d(nan_max_d(s[0], s[1]), nan_max_d(s[2], s[3]));
  return s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(256) void grad_norm_chunk_kernel(const float *__restrict__ g, size_t n, size_t nchunks, int inf,
                                                              double *__restrict__ part) {
  __shared__ double s[4];
  const bool aligned = ((uintptr_t)g & 15) == 0;
  for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const size_t base = c * (size_t)NORM_CHUNK;
    double a = 0.0;
    float mx = 0.0f;
#pragma unroll 4
    for (int k = 0; k < NORM_CHUNK / 1024; ++k) {
      const size_t i0 = base + (size_t)(k * 256 + (int)threadIdx.x) * 4;
      float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (aligned && i0 + 3 < n) {
        const float4 q = *reinterpret_cast<const float4 *>(g + i0);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < n) x[e] = g[i0 + e];
      }
      if (inf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = nan_max(mx, fabsf(x[e]));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) a += (double)x[e] * (double)x[e];
      }
    }
    const double r = norm_block_reduce(a, mx, inf, s);
    if (threadIdx.x == 0) part[c] = r;
  }
}

// per-segment partials: workgroup (j, sgm) takes the j-th of NORM_SEG_SPLIT equal slices of segment sgm = [off[sgm], off[sgm+1])
__global__ __launch_bounds__(256) void grad_norm_seg_kernel(const float *__restrict__ g, size_t n, const int64_t *__restrict__ off, int inf,
                                                            double *__restrict__ seg_part) {
  __shared__ double s[4];
  const int sgm = blockIdx.y, j = blockIdx.x;
  int64_t lo = off[sgm], hi = off[sgm + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > (int64_t)n ? (int64_t)n : hi;       // a table that points outside the buffer reads nothing outside it
  const int64_t len = hi > lo ? hi - lo : 0;
  const int64_t b = lo + len * j / NORM_SEG_SPLIT, e = lo + len * (j + 1) / NORM_SEG_SPLIT;
  double a = 0.0;
  float mx = 0.0f;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) {
    const float x = g[i];
    if (inf) mx = nan_max(mx, fabsf(x));
    else a += (double)x * (double)x;
  }
  const double r = norm_block_reduce(a, mx, inf, s);
  if (threadIdx.x == 0) seg_part[(size_t)sgm * NORM_SEG_SPLIT + j] = r;
}

// chunk partials summed in index order by ONE thread (staged through LDS in tiles); the other threads finish the segments
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double *__restrict__ part, size_t nchunks, int inf, float *__restrict__ total,
                                                              int32_t *__restrict__ nonfinite, const double *__restrict__ seg_part, int nseg,
                                                              float *__restrict__ seg_norms) {
  __shared__ double tile[1024];
  double acc = 0.0;
  for (size_t base = 0; base < nchunks; base += 1024) {
    const int cnt = (int)(nchunks - base < 1024 ? nchunks - base : 1024);
    for (int i = threadIdx.x; i < cnt; i += 256) tile[i] = part[base + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      if (inf) {
        for (int i = 0; i < cnt; ++i) acc = nan_max_d(acc, tile[i]);
      } else {
        // one dependent chain of double adds, in index order; unrolled so that the LDS reads of a group are in flight together and only
        // the adds are serial
#pragma unroll 16
        for (int i = 0; i < cnt; ++i) acc += tile[i];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float t = inf ? (float)acc : (float)sqrt(acc);
    *total = t;
    if (nonfinite) *nonfinite = (__float_as_uint(t) & 0x7f800000u) == 0x7f800000u ? 1 : 0;
  }
  for (int sgm = threadIdx.x; sgm < nseg; sgm += 256) {
    double a = 0.0;
    for (int j = 0; j < NORM_SEG_SPLIT; ++j) {
      const double v = seg_part[(size_t)sgm * NORM_SEG_SPLIT + j];
      a = inf ? nan_max_d(a, v) : a + v;
    }
    seg_norms[sgm] = inf ? (float)a : (float)sqrt(a);
  }
}

// torch's clip coefficient and the step bookkeeping (one thread); the bias corrections are ctcn_adam_step's host expressions, in double
__global__ void clip_control_kernel(ctcn_clip_ctl *__restrict__ c, float max_norm, double lr, double beta1, double beta2, int skip_nonfinite) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float q = max_norm / (c->total_norm + 1e-6f);
  c->clip_coef = q > 1.0f ? 1.0f : q;               // clamp(max=1): a NaN coefficient stays NaN
  int step = c->step;
  if (skip_nonfinite && c->nonfinite) {
    c->skipped += 1;
    c->apply = 0;
  } else {
    step += 1;
    c->step = step;
    c->apply = 1;
  }
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  c->step_size = (float)(lr / bc1);
  c->sqrt_bc2 = (float)sqrt(bc2);
}

// adam_kernel with the gradient scaled by the control block's clip_coef on the way in (g itself is not written) and nothing written at all
// when apply == 0.  g * 1.0f is exact and the decay keeps adam_kernel's fused multiply-add, so clip_coef == 1 gives adam_kernel's bits.
__global__ void adam_ex_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, size_t n,
                               float beta1, float beta2, float eps, float wd, const ctcn_clip_ctl *__restrict__ c) {
  if (c->apply == 0) return;
  const float clip = c->clip_coef, step_size = c->step_size, sqrt_bc2 = c->sqrt_bc2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float gc = g[i] * clip;
    const float gv = __builtin_fmaf(wd, pv, gc);      // adam_kernel's contraction of g + wd * p, written out: not the optimiser's choice here
    const float mv = beta1 * m[i] + (1.0f - beta1) * gv;
    const float vv = beta2 * v[i] + (1.0f - beta2) * gv * gv;
    m[i] = mv; v[i] = vv;
    p[i] = pv - step_size * (mv / (sqrtf(vv) / sqrt_bc2 + eps));
  }
}

// x[i] *= *scalar (a NaN scalar poisons x, as torch's clip_grad_norm_ does with a non-finite norm): 16 B per lane where x allows it
__global__ void scale_by_scalar_kernel(float *__restrict__ x, size_t n, const float *__restrict__ scalar) {
  const float sc = *scalar;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  if (((uintptr_t)x & 15) == 0) {
    const size_t n4 = n / 4;
    for (size_t i = tid; i < n4; i += nthr) {
      float4 q = reinterpret_cast<float4 *>(x)[i];
      q.x *= sc; q.y *= sc; q.z *= sc; q.w *= sc;
      reinterpret_cast<float4 *>(x)[i] = q;
    }
    for (size_t i = n4 * 4 + tid; i < n; i += nthr) x[i] *= sc;
  } else {
    for (size_t i = tid; i < n; i += nthr) x[i] *= sc;
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

extern "C" size_t ctcn_grad_norm_ws_bytes(size_t n, int nseg) {
  if (nseg < 0) return 0;
  return (ceil_div_z(n, NORM_CHUNK) + (size_t)nseg * NORM_SEG_SPLIT) * sizeof(double);
}

extern "C" int ctcn_grad_norm(const float *g, size_t n, int norm_type, const int64_t *seg_offsets, int nseg, float *seg_norms,
                              float *total_norm, int32_t *nonfinite, int grid_blocks, void *ws, size_t ws_bytes, void *stream) {
  CTCN_REQUIRE(g && total_norm, "ctcn_grad_norm: null pointer");
  CTCN_REQUIRE(norm_type == CTCN_NORM_L2 || norm_type == CTCN_NORM_INF, "ctcn_grad_norm: norm_type %d (CTCN_NORM_L2 or CTCN_NORM_INF)", norm_type);
  CTCN_REQUIRE(nseg >= 0 && grid_blocks >= 0 && (nseg == 0 || (seg_offsets && seg_norms)), "ctcn_grad_norm: bad segment table / grid");
  const size_t need = ctcn_grad_norm_ws_bytes(n, nseg);
  if (need > 0 && (!ws || ws_bytes < need || ((uintptr_t)ws & 7))) {
    ctcn_set_error("ctcn_grad_norm: workspace of %zu bytes, 8-byte aligned, needed (got %zu)", need, ws_bytes);
    return CTCN_EWORKSPACE;
  }
  const size_t nchunks = ceil_div_z(n, NORM_CHUNK);
  double *part = (double *)ws, *seg_part = part + nchunks;
  const int inf = norm_type == CTCN_NORM_INF;
  if (nchunks > 0) {
    const size_t cap = grid_blocks > 0 ? (size_t)grid_blocks : (size_t)std::max(ctcn_device_cus(), 1) * 8;
    hipLaunchKernelGGL(grad_norm_chunk_kernel, dim3((unsigned)std::min(nchunks, cap)), dim3(256), 0, (hipStream_t)stream, g, n, nchunks, inf, part);
    CTCN_LAUNCH_CHECK();
  }
  if (nseg > 0) {
    hipLaunchKernelGGL(grad_norm_seg_kernel, dim3(NORM_SEG_SPLIT, nseg), dim3(256), 0, (hipStream_t)stream, g, n, seg_offsets, inf, seg_part);
    CTCN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nchunks, inf, total_norm, nonfinite, seg_part, nseg,
                     seg_norms);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_clip_control(ctcn_clip_ctl *ctl, float max_norm, float lr, float beta1, float beta2, int skip_nonfinite, void *stream) {
  CTCN_REQUIRE(ctl && ((uintptr_t)ctl & 3) == 0, "ctcn_clip_control: null / misaligned control block");
  CTCN_REQUIRE(max_norm > 0.0f, "ctcn_clip_control: max_norm must be > 0 (+inf: no clipping)");
  hipLaunchKernelGGL(clip_control_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, max_norm, (double)lr, (double)beta1, (double)beta2,
                     skip_nonfinite != 0);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_adam_step_ex(float *p, const float *g, float *m, float *v, size_t n, float beta1, float beta2, float eps,
                                 float weight_decay, const ctcn_clip_ctl *ctl, void *stream) {
  CTCN_REQUIRE(p && g && m && v && ctl, "ctcn_adam_step_ex: null pointer");
  if (n == 0) return CTCN_OK;
  const int blocks = (int)std::min((size_t)4096, ceil_div_z(n, 256));
  hipLaunchKernelGGL(adam_ex_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, beta1, beta2, eps, weight_decay, ctl);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_scale_by_device_scalar(float *x, size_t n, const float *scalar, void *stream) {
  CTCN_REQUIRE(x && scalar, "ctcn_scale_by_device_scalar: null pointer");
  if (n == 0) return CTCN_OK;
  const int blocks = (int)std::min((size_t)std::max(ctcn_device_cus(), 1) * 8, ceil_div_z(ceil_div_z(n, 4), 256));
  hipLaunchKernelGGL(scale_by_scalar_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, n, scalar);
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
