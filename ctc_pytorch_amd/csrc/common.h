// common.h -- shared helpers for the gfx950 kernels of libctcn.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/ctcn.h"

void ctcn_set_error(const char *fmt, ...);
int *ctcn_status_word(void);      // device int registered with ctcn_set_status_buffer (may be null)
int ctcn_opt_rnn_persistent(void);
int ctcn_transpose01_pair(const float *in0, const float *in1, float *out0, float *out1, int A, int B, int C, void *stream);   // two ctcn_transpose01 in one launch
// What a sequence of internal bf16x3 GEMM calls left in ITS workspace, owned by the function that makes the sequence (on its stack: no state
// outlives an ABI call or is shared between threads -- round 3): a call records which operand planes it wrote, and a call
// made with `same_a` / `same_b` set (one-shot requests: "the operand is the one of my previous call, unmodified") skips that split pass
// when pointer / shape / layout / workspace / stream match.
struct GemmPlanes {
  const float *A = nullptr; int lda = 0, M = 0, Ka = 0, transA = 0; void *ws_a = nullptr, *st_a = nullptr; bool a_valid = false;
  const float *B = nullptr; int ldb = 0, N = 0, Kb = 0, transB = 0, shift = 0; void *ws_b = nullptr, *st_b = nullptr; const void *bh = nullptr; bool b_valid = false;
  bool same_a = false, same_b = false;
};
int ctcn_gemm_on_xcds(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C,
                      int ldc, float beta, int precision, void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow, GemmPlanes *planes = nullptr);
int ctcn_gemm_shift_b(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, float beta, int precision,
                      void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow, int shift, GemmPlanes *planes = nullptr);
int ctcn_opt_handoff(void);
int ctcn_opt_poll_depth(void);
int ctcn_opt_bwd_scatter(void);
int ctcn_opt_handoff_tags(void);
int ctcn_opt_side_split_wgs(void);
int ctcn_opt_gemm_big_tiles(void);
int ctcn_opt_recurrence_only(void);   // measurement aid: ctcn_rnn_fwd/bwd skip their GEMMs (results are NOT valid)

#define CTCN_REQUIRE(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      ctcn_set_error(__VA_ARGS__);       \
      return CTCN_EINVAL;                \
    }                                    \
  } while (0)

#define CTCN_HIP(expr)                                                                   \
  do {                                                                                   \
    hipError_t e__ = (expr);                                                             \
    if (e__ != hipSuccess) {                                                             \
      ctcn_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
      return CTCN_EHIP;                                                                  \
    }                                                                                    \
  } while (0)

#define CTCN_LAUNCH_CHECK() CTCN_HIP(hipGetLastError())

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t ceil_div_z(size_t a, size_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// Workgroup barrier for LDS hand-offs only.  __syncthreads() carries a workgroup-scope fence that drains EVERY
// outstanding global load / store of the wave (s_waitcnt vmcnt(0)); kernels with a serial inner loop (recurrences, the CTC lattice)
// keep operand prefetches and result stores in flight across their LDS barriers, so they wait for LDS traffic only.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Sample i of a waveform batch of float32 or int16 samples (the front-end's wave / wave_is_int16 pair): int16 is converted where it is read.
// Host callable: the host twins read their input the same way.
__host__ __device__ __forceinline__ float wave_sample(const void *wave, int is_i16, size_t i) {
  return is_i16 ? (float)static_cast<const int16_t *>(wave)[i] : static_cast<const float *>(wave)[i];
}

// Philox4x32-10 (Salmon et al., SC'11): counter = element-group index, key = seed.  (Host callable too: specaug.hip's host twin draws from it.)
__host__ __device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
#else
  const uint32_t hi0 = (uint32_t)(((uint64_t)M0 * c[0]) >> 32), lo0 = M0 * c[0];
  const uint32_t hi1 = (uint32_t)(((uint64_t)M1 * c[2]) >> 32), lo1 = M1 * c[2];
#endif
  const uint32_t n0 = hi1 ^ c[1] ^ k[0], n1 = lo1, n2 = hi0 ^ c[3] ^ k[1], n3 = lo0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
  k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
}
__host__ __device__ __forceinline__ void philox4(uint64_t seed, uint64_t ctr, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
  for (int i = 0; i < 10; ++i) philox_round(c, k);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = c[i];
}

// round-to-nearest-even f32 -> bf16 (bits)
__device__ __forceinline__ unsigned short f2bf(float f) {      // round to nearest even: one v_cvt_pk_bf16_f32 on gfx950
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}
