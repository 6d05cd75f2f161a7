// gemm.hip -- MFMA GEMM for gfx950 (MI355X).
//
// C[M,N] = op(A)[M,K] * op(B)[K,N] + beta*C, row-major, arbitrary M/N/K/strides.
// replaces: nn.Linear(2H,V,bias=False) (reference timit/models/model_ctc.py:137,166) and the time-parallel
// input projections X*W_ih^T of nn.LSTM/GRU/RNN (model_ctc.py:33), plus their dgrad/wgrad GEMMs.
//
// Design (wave64, 4 SIMDs/CU):
//   * 128x128 output tile per 256-thread workgroup, 4 waves as 2x2, each wave a 64x64 sub-tile =
//     2x2 MFMA tiles of v_mfma_f32_32x32x2_f32 (exact f32 == fmaf chain) -> 64 accumulator VGPRs.
//   * BK=16 K-slab staged through LDS in k-major order ([k][m] / [k][n]) so that a wave's MFMA operand
//     fetch (lane l reads element (m = l&31, k = l>>5)) is a conflict-free ds_read_b32 of 32 consecutive
//     floats per half-wave; row pad +4 floats keeps the transposing stores <= 2-way conflicted.
//   * global -> register -> LDS staging with the next slab's global loads issued before the MFMAs of the
//     current slab (register prefetch), float4 (16 B/lane) global loads when the operand is 16-B aligned.
//   * deterministic split-K (grid.z) through a caller-provided workspace + a second reduce pass, used when
//     the M*N tile grid alone cannot fill the 256 CUs (weight-gradient GEMMs, K = T*B = 25 600).
//   * XCD-aware tile order: consecutive workgroup ids are dealt round-robin to the 8 XCDs, so the remap
//     gives each XCD a contiguous band of M-tiles that share the same B panel in its private L2.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 16, PAD = 4;

// XCD-aware tile order (bijective for any tile count): blocks b, b + 8, b + 16, ... share an XCD / L2; each XCD gets a contiguous band of tiles
__device__ __forceinline__ int xcd_band_tile(int bid, int nt) {
  const int xcd = bid & 7, q = nt >> 3, r = nt & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
// ---- global -> registers (8 floats per thread per operand slab) --------------------------------
// KC: operand element (r, k) at src[(r0+r)*ld + k0+k]  (k contiguous)
__device__ __forceinline__ void g2r_kc(const float *__restrict__ src, int ld, int r0, int R, int k0, int Kend,
                                       bool vec, int tid, float (&reg)[8]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j;
    const int r = idx >> 2, kq = (idx & 3) * 4;
    const int gr = r0 + r, gk = k0 + kq;
    const float *p = src + (size_t)gr * ld + gk;
    if (vec && gr < R && gk + 3 < Kend) {
      const float4 v = *reinterpret_cast<const float4 *>(p);
      reg[4 * j + 0] = v.x; reg[4 * j + 1] = v.y; reg[4 * j + 2] = v.z; reg[4 * j + 3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) reg[4 * j + c] = (gr < R && gk + c < Kend) ? p[c] : 0.0f;
    }
  }
}
__device__ __forceinline__ void r2s_kc(float (*s)[BM + PAD], int tid, const float (&reg)[8]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j;
    const int r = idx >> 2, kq = (idx & 3) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) s[kq + c][r] = reg[4 * j + c];
  }
}
// MC: operand element (r, k) at src[(k0+k)*ld + r0+r]  (r contiguous)
__device__ __forceinline__ void g2r_mc(const float *__restrict__ src, int ld, int r0, int R, int k0, int Kend,
                                       bool vec, int tid, float (&reg)[8]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j;
    const int k = idx >> 5, rq = (idx & 31) * 4;
    const int gk = k0 + k, gr = r0 + rq;
    const float *p = src + (size_t)gk * ld + gr;
    if (vec && gk < Kend && gr + 3 < R) {
      const float4 v = *reinterpret_cast<const float4 *>(p);
      reg[4 * j + 0] = v.x; reg[4 * j + 1] = v.y; reg[4 * j + 2] = v.z; reg[4 * j + 3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) reg[4 * j + c] = (gk < Kend && gr + c < R) ? p[c] : 0.0f;
    }
  }
}
__device__ __forceinline__ void r2s_mc(float (*s)[BM + PAD], int tid, const float (&reg)[8]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j;
    const int k = idx >> 5, rq = (idx & 31) * 4;
    *reinterpret_cast<float4 *>(&s[k][rq]) = make_float4(reg[4 * j], reg[4 * j + 1], reg[4 * j + 2], reg[4 * j + 3]);
  }
}

// TA: A stored [K][M] (m contiguous).  TB: B stored [N][K] (k contiguous).
// one 128x128 output tile (`bid`) of K-split `split`
template <bool TA, bool TB>
__device__ __forceinline__ void f32_tile(float (*sA)[BM + PAD], float (*sB)[BN + PAD], int bid, int split, int M, int N, int K,
                                         const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb, float *__restrict__ C,
                                         int ldc, float beta, int kchunk, float *__restrict__ ws, int tiles_n, bool vecA, bool vecB) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;   // consecutive ids walk N first: share the A panel
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  float ra[8], rb[8];
  auto loadA = [&](int k0) {
    if (TA) g2r_mc(A, lda, m0, M, k0, kend, vecA, tid, ra);
    else g2r_kc(A, lda, m0, M, k0, kend, vecA, tid, ra);
  };
  auto loadB = [&](int k0) {
    if (TB) g2r_kc(B, ldb, n0, N, k0, kend, vecB, tid, rb);
    else g2r_mc(B, ldb, n0, N, k0, kend, vecB, tid, rb);
  };
  if (kbeg < kend) {
    loadA(kbeg);
    loadB(kbeg);
  }
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    __syncthreads();   // previous slab fully consumed
    if (TA) r2s_mc(sA, tid, ra); else r2s_kc(sA, tid, ra);
    if (TB) r2s_kc(sB, tid, rb); else r2s_mc(sB, tid, rb);
    __syncthreads();
    if (k0 + BK < kend) {   // prefetch next slab into registers while the MFMAs run
      loadA(k0 + BK);
      loadB(k0 + BK);
    }
    const int kl = lane >> 5, ml = lane & 31;
#pragma unroll
    for (int k = 0; k < BK; k += 2) {
      const float a0 = sA[k + kl][wm * 64 + ml], a1 = sA[k + kl][wm * 64 + 32 + ml];
      const float b0 = sB[k + kl][wn * 64 + ml], b1 = sB[k + kl][wn * 64 + 32 + ml];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  float *out = ws ? ws + (size_t)split * M * N : C;
  const int ldo = ws ? N : ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < M && col < N) {
          float v = acc[i][j][e];
          float *p = out + (size_t)row * ldo + col;
          if (!ws && beta != 0.0f) v += beta * *p;
          *p = v;
        }
      }
    }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_f32_kernel(int M, int N, int K, const float *__restrict__ A, int lda,
                                                       const float *__restrict__ B, int ldb, float *__restrict__ C,
                                                       int ldc, float beta, int kchunk, float *__restrict__ ws,
                                                       int tiles_m, int tiles_n, bool vecA, bool vecB) {
  __shared__ __attribute__((aligned(16))) float sA[BK][BM + PAD];
  __shared__ __attribute__((aligned(16))) float sB[BK][BN + PAD];
  const int bid = xcd_band_tile(blockIdx.x, tiles_m * tiles_n);
  f32_tile<TA, TB>(sA, sB, bid, blockIdx.y, M, N, K, A, lda, B, ldb, C, ldc, beta, kchunk, ws, tiles_n, vecA, vecB);
}

// XCD-filtered variant for the weight-gradient side stream (see gemm_planes_nt_queue_kernel)
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_f32_queue_kernel(int M, int N, int K, const float *__restrict__ A, int lda,
                                                             const float *__restrict__ B, int ldb, float *__restrict__ C, int ldc,
                                                             float beta, int kchunk, float *__restrict__ ws, int tiles_m, int tiles_n,
                                                             bool vecA, bool vecB, int splits, unsigned xcd_allow,
                                                             unsigned *__restrict__ queue) {
  __shared__ __attribute__((aligned(16))) float sA[BK][BM + PAD];
  __shared__ __attribute__((aligned(16))) float sB[BK][BN + PAD];
  __shared__ int s_item;
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  if (!((xcd_allow >> (x & 15)) & 1u)) return;
  const int nt = tiles_m * tiles_n, total = nt * splits;
  for (;;) {
    if (threadIdx.x == 0) s_item = (int)atomicAdd(queue, 1u);
    __syncthreads();
    const int item = s_item;
    if (item >= total) return;
    f32_tile<TA, TB>(sA, sB, item % nt, item / nt, M, N, K, A, lda, B, ldb, C, ldc, beta, kchunk, ws, tiles_n, vecA, vecB);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// precision = 1: split-operand bf16 MFMA ("bf16x3").  Every f32 operand is split on the fly into
// hi = bf16(x), lo = bf16(x - hi) while it is staged into LDS, and the product is accumulated in f32 as
// a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_bf16 (3 MFMAs = 96 cycles per 32x32x16 instead of
// 8 x 64 = 512 cycles of f32 MFMA).  16 mantissa bits per operand -> relative error ~2^-16 per product, i.e.
// f32-class results (max-abs 1e-5 on unit-scale data) at ~5x the f32-MFMA rate.
// LDS image: [row][k] with k contiguous (8 bf16 = one ds_read_b128 MFMA fragment), row stride 40 bf16 = 80 B so the
// 16 lanes of a read group land on 16 distinct 16-B bank slots.
// ------------------------------------------------------------------------------------------------
constexpr int XBK = 32, XLD = 40;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_bf16(float x, unsigned short &hi, unsigned short &lo) {
  hi = f2bf(x);
  lo = f2bf(x - __uint_as_float((unsigned)hi << 16));
}

// KC: element (r,k) at src[(r0+r)*ld + k0+k];  16 floats per thread: 4 x float4 along k
__device__ __forceinline__ void x_g2r_kc(const float *__restrict__ src, int ld, int r0, int R, int k0, int Kend, bool vec,
                                         int tid, float (&reg)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + 256 * j;
    const int r = idx >> 3, kq = (idx & 7) * 4;
    const int gr = r0 + r, gk = k0 + kq;
    const float *p = src + (size_t)gr * ld + gk;
    if (vec && gr < R && gk + 3 < Kend) {
      const float4 v = *reinterpret_cast<const float4 *>(p);
      reg[4 * j] = v.x; reg[4 * j + 1] = v.y; reg[4 * j + 2] = v.z; reg[4 * j + 3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) reg[4 * j + c] = (gr < R && gk + c < Kend) ? p[c] : 0.0f;
    }
  }
}
__device__ __forceinline__ void x_r2s_kc(unsigned short (*sh)[XLD], unsigned short (*sl)[XLD], int tid, const float (&reg)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + 256 * j;
    const int r = idx >> 3, kq = (idx & 7) * 4;
    unsigned short h[4], l[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) split_bf16(reg[4 * j + c], h[c], l[c]);
    *reinterpret_cast<uint2 *>(&sh[r][kq]) = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    *reinterpret_cast<uint2 *>(&sl[r][kq]) = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
  }
}
// MC: element (r,k) at src[(k0+k)*ld + r0+r];  4 x float4 along r, transposed into the [row][k] image
__device__ __forceinline__ void x_g2r_mc(const float *__restrict__ src, int ld, int r0, int R, int k0, int Kend, bool vec,
                                         int tid, float (&reg)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + 256 * j;
    const int k = idx >> 5, rq = (idx & 31) * 4;
    const int gk = k0 + k, gr = r0 + rq;
    const float *p = src + (size_t)gk * ld + gr;
    if (vec && gk < Kend && gr + 3 < R) {
      const float4 v = *reinterpret_cast<const float4 *>(p);
      reg[4 * j] = v.x; reg[4 * j + 1] = v.y; reg[4 * j + 2] = v.z; reg[4 * j + 3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) reg[4 * j + c] = (gk < Kend && gr + c < R) ? p[c] : 0.0f;
    }
  }
}
__device__ __forceinline__ void x_r2s_mc(unsigned short (*sh)[XLD], unsigned short (*sl)[XLD], int tid, const float (&reg)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + 256 * j;
    const int k = idx >> 5, rq = (idx & 31) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned short h, l;
      split_bf16(reg[4 * j + c], h, l);
      sh[rq + c][k] = h;
      sl[rq + c][k] = l;
    }
  }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_bf16x3_kernel(int M, int N, int K, const float *__restrict__ A, int lda,
                                                          const float *__restrict__ B, int ldb, float *__restrict__ C,
                                                          int ldc, float beta, int kchunk, float *__restrict__ ws,
                                                          int tiles_m, int tiles_n, bool vecA, bool vecB) {
  __shared__ __attribute__((aligned(16))) unsigned short sAh[BM][XLD], sAl[BM][XLD], sBh[BN][XLD], sBl[BN][XLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int bid = xcd_band_tile(blockIdx.x, tiles_m * tiles_n);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  float ra[16], rb[16];
  auto loadA = [&](int k0) {
    if (TA) x_g2r_mc(A, lda, m0, M, k0, kend, vecA, tid, ra);
    else x_g2r_kc(A, lda, m0, M, k0, kend, vecA, tid, ra);
  };
  auto loadB = [&](int k0) {
    if (TB) x_g2r_kc(B, ldb, n0, N, k0, kend, vecB, tid, rb);
    else x_g2r_mc(B, ldb, n0, N, k0, kend, vecB, tid, rb);
  };
  if (kbeg < kend) { loadA(kbeg); loadB(kbeg); }
  for (int k0 = kbeg; k0 < kend; k0 += XBK) {
    __syncthreads();
    if (TA) x_r2s_mc(sAh, sAl, tid, ra); else x_r2s_kc(sAh, sAl, tid, ra);
    if (TB) x_r2s_kc(sBh, sBl, tid, rb); else x_r2s_mc(sBh, sBl, tid, rb);
    __syncthreads();
    if (k0 + XBK < kend) { loadA(k0 + XBK); loadB(k0 + XBK); }
    const int ml = lane & 31, kg = (lane >> 5) * 8;
#pragma unroll
    for (int ks = 0; ks < XBK; ks += 16) {
      bf16x8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *reinterpret_cast<const bf16x8_t *>(&sAh[wm * 64 + i * 32 + ml][ks + kg]);
        al[i] = *reinterpret_cast<const bf16x8_t *>(&sAl[wm * 64 + i * 32 + ml][ks + kg]);
        bh[i] = *reinterpret_cast<const bf16x8_t *>(&sBh[wn * 64 + i * 32 + ml][ks + kg]);
        bl[i] = *reinterpret_cast<const bf16x8_t *>(&sBl[wn * 64 + i * 32 + ml][ks + kg]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);   // small terms first
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
  }
  float *out = ws ? ws + (size_t)blockIdx.y * M * N : C;
  const int ldo = ws ? N : ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < M && col < N) {
          float v = acc[i][j][e];
          float *p = out + (size_t)row * ldo + col;
          if (!ws && beta != 0.0f) v += beta * *p;
          *p = v;
        }
      }
    }
}

// ------------------------------------------------------------------------------------------------
// precision = 1, main path: bf16x3 on PRE-SPLIT operand planes.
//   1. one HBM-bound pass per operand splits the f32 matrix into hi/lo bf16 planes laid out [rows][Kp] with the
//      contraction index contiguous and zero-padded to a multiple of 64 (the pass transposes when the operand is
//      stored contraction-major), so that
//   2. a single "NT" kernel  C[m,n] = sum_k A[m,k] * B[n,k]  serves all four transpose cases with no conversion and
//      no transposition in its inner loop: 128x128x64 tiles, 16-B global loads -> XOR-swizzled LDS rows of 128 B
//      (conflict-free ds_write_b128 / ds_read_b128: slot = 8*(row&1) + (chunk ^ ((row>>1)&7))), register prefetch of
//      the next K-slab, 3 x v_mfma_f32_32x32x16_bf16 per fragment pair (lo*hi, hi*lo, hi*hi), f32 accumulate.
// ------------------------------------------------------------------------------------------------
constexpr int PBK = 64;

__global__ void split_rows_kernel(const float *__restrict__ src, int ld, int R, int C, int Cp, unsigned short *__restrict__ hi,
                                  unsigned short *__restrict__ lo) {
  // out[r][c] (row stride Cp) = split(src[r*ld + c]), zero for c >= C; 4 elements per thread
  const size_t total = (size_t)R * (Cp / 4);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / (Cp / 4)), c = (int)(i - (size_t)r * (Cp / 4)) * 4;
    unsigned short h[4], l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = (c + k < C) ? src[(size_t)r * ld + c + k] : 0.0f;
      split_bf16(v, h[k], l[k]);
    }
    *reinterpret_cast<uint2 *>(hi + (size_t)r * Cp + c) = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    *reinterpret_cast<uint2 *>(lo + (size_t)r * Cp + c) = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
  }
}

// out[c][r] (row stride Rp) = split(src[r*ld + c]); 64x64 tiles through LDS; zero for r >= R (k padding)
// shift: output row k takes source row k - shift when that lies in [0, R), zero otherwise (a matrix delayed / advanced by
// |shift| contraction steps: h_prev of the recurrent weight gradient)
__device__ __forceinline__ void split_transpose_tile(float (*t)[65], int bx, int by, const float *__restrict__ src, int ld, int R, int C, int Rp,
                                                     unsigned short *__restrict__ hi, unsigned short *__restrict__ lo, int shift) {
  const int r0 = by * 64, c0 = bx * 64;
  const int tid = threadIdx.x;
  // fast path (every large operand): 16-B global loads along the columns, 16-B plane stores along the rows (8 bf16 of one
  // output row per lane: a wave writes eight 128-B runs), LDS image padded to 65 floats so that both the row-wise scalar
  // writes and the column-wise reads are conflict-free.  8 global instructions per thread instead of 48.
  const bool vec = c0 + 64 <= C && (ld & 3) == 0 && ((uintptr_t)src & 15) == 0;
  if (vec) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + 256 * j, i = idx >> 4, c4 = idx & 15;
      const int r = r0 + i - shift;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r >= 0 && r < R && r0 + i < R) v = *reinterpret_cast<const float4 *>(src + (size_t)r * ld + c0 + 4 * c4);
      t[i][4 * c4 + 0] = v.x; t[i][4 * c4 + 1] = v.y; t[i][4 * c4 + 2] = v.z; t[i][4 * c4 + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int g = tid + 256 * j, c = g >> 3, ro = g & 7;
      unsigned hw[4], lw[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned short h0, l0, h1, l1;
        split_bf16(t[ro * 8 + 2 * e][c], h0, l0);
        split_bf16(t[ro * 8 + 2 * e + 1][c], h1, l1);
        hw[e] = (unsigned)h0 | ((unsigned)h1 << 16);
        lw[e] = (unsigned)l0 | ((unsigned)l1 << 16);
      }
      const size_t o = (size_t)(c0 + c) * Rp + r0 + ro * 8;
      *reinterpret_cast<uint4 *>(hi + o) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
      *reinterpret_cast<uint4 *>(lo + o) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    }
    return;
  }
  const int tx = tid & 63, ty = tid >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i - shift, c = c0 + tx;
    t[i][tx] = (r >= 0 && r < R && r0 + i < R && c < C) ? src[(size_t)r * ld + c] : 0.0f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < Rp) {
      unsigned short h, l;
      split_bf16(t[tx][i], h, l);
      hi[(size_t)c * Rp + r] = h;
      lo[(size_t)c * Rp + r] = l;
    }
  }
}

__global__ __launch_bounds__(256) void split_transpose_kernel(const float *__restrict__ src, int ld, int R, int C, int Rp,
                                                              unsigned short *__restrict__ hi, unsigned short *__restrict__ lo, int shift) {
  __shared__ float t[64][65];
  split_transpose_tile(t, blockIdx.x, blockIdx.y, src, ld, R, C, Rp, hi, lo, shift);
}
// XCD-filtered variant (see gemm_planes_nt_queue_kernel): tiles come from an atomic queue, workgroups off `xcd_allow` exit
__global__ __launch_bounds__(256) void split_transpose_queue_kernel(const float *__restrict__ src, int ld, int R, int C, int Rp,
                                                                    unsigned short *__restrict__ hi, unsigned short *__restrict__ lo, int tiles_x,
                                                                    int tiles_y, unsigned xcd_allow, unsigned *__restrict__ queue, int shift) {
  __shared__ float t[64][65];
  __shared__ int s_item;
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  if (!((xcd_allow >> (x & 15)) & 1u)) return;
  for (;;) {
    if (threadIdx.x == 0) s_item = (int)atomicAdd(queue, 1u);
    __syncthreads();
    const int item = s_item;
    if (item >= tiles_x * tiles_y) return;
    split_transpose_tile(t, item % tiles_x, item / tiles_x, src, ld, R, C, Rp, hi, lo, shift);
    __syncthreads();
  }
}

__device__ __forceinline__ int pswz(int row, int kc) { return row * 128 + ((kc ^ ((row >> 1) & 7)) << 4); }   // byte offset in a plane tile

// One (64*TI) x (64*TJ) output tile (`bid`) of K-split `split`.  2 x 2 waves, each owning (32*TI) x (32*TJ) = TI x TJ
// MFMA tiles: per 16-k step a wave reads 2*(TI + TJ) fragments from LDS for 3*TI*TJ MFMAs, so the LDS traffic per MFMA
// falls from 0.67 fragments (TI = TJ = 2) to 0.5 (2 x 4 / 4 x 2) -- the 128x128 kernel is LDS-bound, not MFMA-bound.
// sm = dynamic LDS: [Ah | Al] (64*TI rows x 128 B each) then [Bh | Bl] (64*TJ rows x 128 B each).
// Measured and dropped: 32-k stages (32 KB of LDS, 156 VGPRs: three workgroups per CU instead of two) -- bit-identical, 1-4 %
// slower (dx 25 600 x 640 x 2 560: 436 vs 418 us with its split passes), so occupancy is not what holds the 128x128 tile at
// ~36 % of the MFMA rate; PMC (profiles/r01_pmc_gemm_probe_v10.txt): the A planes cross the fabric 2.3 x per XCD.
template <int TI, int TJ>
__device__ __forceinline__ void plane_tile(unsigned char *sm, int bid, int split, int M, int N, int Kp,
                                           const unsigned short *__restrict__ Ah, const unsigned short *__restrict__ Al,
                                           const unsigned short *__restrict__ Bh, const unsigned short *__restrict__ Bl,
                                           float *__restrict__ C, int ldc, float beta, int kchunk, float *__restrict__ ws, int tiles_n) {
  constexpr int TBM = 64 * TI, TBN = 64 * TJ;
  constexpr int CA = TBM * 8 / 256, CB = TBN * 8 / 256;              // 16-B staging chunks per thread and plane
  unsigned char *sAh = sm, *sAl = sm + TBM * 128, *sBh = sm + 2 * TBM * 128, *sBl = sBh + TBN * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * TBM, n0 = tn * TBN;
  const int kbeg = split * kchunk;
  const int kend = min(Kp, kbeg + kchunk);

  f32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // element offsets of this thread's chunks in the A-side and B-side planes (rows clamped: out-of-range rows are never stored)
  unsigned offA[CA], offB[CB];
#pragma unroll
  for (int j = 0; j < CA; ++j) offA[j] = (unsigned)min(m0 + ((tid + 256 * j) >> 3), M - 1) * (unsigned)Kp + ((tid + 256 * j) & 7) * 8;
#pragma unroll
  for (int j = 0; j < CB; ++j) offB[j] = (unsigned)min(n0 + ((tid + 256 * j) >> 3), N - 1) * (unsigned)Kp + ((tid + 256 * j) & 7) * 8;
  u32x4 pAh[CA], pAl[CA], pBh[CB], pBl[CB];      // ext-vector values (arrays of HIP's uint4 class end up in scratch)
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      pAh[j] = *reinterpret_cast<const u32x4 *>(Ah + offA[j] + k0);
      pAl[j] = *reinterpret_cast<const u32x4 *>(Al + offA[j] + k0);
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      pBh[j] = *reinterpret_cast<const u32x4 *>(Bh + offB[j] + k0);
      pBl[j] = *reinterpret_cast<const u32x4 *>(Bl + offB[j] + k0);
    }
  };
  if (kbeg < kend) gload(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += PBK) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      const int so = pswz((tid + 256 * j) >> 3, (tid + 256 * j) & 7);
      *reinterpret_cast<u32x4 *>(sAh + so) = pAh[j];
      *reinterpret_cast<u32x4 *>(sAl + so) = pAl[j];
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int so = pswz((tid + 256 * j) >> 3, (tid + 256 * j) & 7);
      *reinterpret_cast<u32x4 *>(sBh + so) = pBh[j];
      *reinterpret_cast<u32x4 *>(sBl + so) = pBl[j];
    }
    __syncthreads();
    if (k0 + PBK < kend) gload(k0 + PBK);
    const int ml = lane & 31, g = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kc = ks * 2 + g;
      bf16x8_t ah[TI], al[TI], bh[TJ], bl[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        const int ra = wm * 32 * TI + i * 32 + ml;
        ah[i] = *reinterpret_cast<const bf16x8_t *>(sAh + pswz(ra, kc));
        al[i] = *reinterpret_cast<const bf16x8_t *>(sAl + pswz(ra, kc));
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int rb = wn * 32 * TJ + j * 32 + ml;
        bh[j] = *reinterpret_cast<const bf16x8_t *>(sBh + pswz(rb, kc));
        bl[j] = *reinterpret_cast<const bf16x8_t *>(sBl + pswz(rb, kc));
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);   // small terms first
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
  }
  float *out = ws ? ws + (size_t)split * M * N : C;
  const int ldo = ws ? N : ldc;
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int col = n0 + wn * 32 * TJ + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 32 * TI + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < M && col < N) {
          float v = acc[i][j][e];
          float *p = out + (size_t)row * ldo + col;
          if (!ws && beta != 0.0f) v += beta * *p;
          *p = v;
        }
      }
    }
}

template <int TI, int TJ>
__global__ __launch_bounds__(256) void gemm_planes_nt_kernel(int M, int N, int Kp, const unsigned short *__restrict__ Ah,
                                                             const unsigned short *__restrict__ Al, const unsigned short *__restrict__ Bh,
                                                             const unsigned short *__restrict__ Bl, float *__restrict__ C, int ldc, float beta,
                                                             int kchunk, float *__restrict__ ws, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char psm[];       // Ah | Al | Bh | Bl tiles
  const int bid = xcd_band_tile(blockIdx.x, tiles_m * tiles_n);
  plane_tile<TI, TJ>(psm, bid, blockIdx.y, M, N, Kp, Ah, Al, Bh, Bl, C, ldc, beta, kchunk, ws, tiles_n);
}

// Same GEMM for a side stream that must stay off the XCDs a persistent recurrence is running on: workgroups that wake up
// on an XCD outside `xcd_allow` (bit x = XCD x, read from HW_REG_XCC_ID) exit at once, the others pull (tile, split)
// items from an atomic queue until it is empty.  The launch is sized to fill the allowed XCDs, not the tile count.
template <int TI, int TJ>
__global__ __launch_bounds__(256) void gemm_planes_nt_queue_kernel(int M, int N, int Kp, const unsigned short *__restrict__ Ah,
                                                                   const unsigned short *__restrict__ Al, const unsigned short *__restrict__ Bh,
                                                                   const unsigned short *__restrict__ Bl, float *__restrict__ C, int ldc,
                                                                   float beta, int kchunk, float *__restrict__ ws, int tiles_m, int tiles_n,
                                                                   int splits, unsigned xcd_allow, unsigned *__restrict__ queue) {
  extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
  __shared__ int s_item;
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  if (!((xcd_allow >> (x & 15)) & 1u)) return;
  const int nt = tiles_m * tiles_n, total = nt * splits;
  for (;;) {
    if (threadIdx.x == 0) s_item = (int)atomicAdd(queue, 1u);
    __syncthreads();
    const int item = s_item;
    if (item >= total) return;
    plane_tile<TI, TJ>(psm, item % nt, item / nt, M, N, Kp, Ah, Al, Bh, Bl, C, ldc, beta, kchunk, ws, tiles_n);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// 256 x 256 / 256 x 128 plane tiles for the activation-sized products (M = T*B rows).
// The 128 x 128 tile above moves 64 KB of planes through a CU per 64-k slab for 3 x 128 x 128 x 64 MACs: at the MFMA rate that
// is ~42 B/clk per CU out of an L2 that delivers ~56, so the kernel is L2-bandwidth bound at ~36 % of the MFMA rate (and the A
// planes cross the fabric 2.3 x per XCD).  A 256 x 256 tile halves the bytes per MAC (21 B/clk), a 256 x 128 tile takes 31.
//   * 512 threads = 8 waves as 2 (M) x 4 (N); a wave owns 128 x 64 (or 128 x 32) outputs = 4 x WNT MFMA tiles of 32 x 32: 128 / 64
//     accumulator VGPRs; per 16-k step 8 + 4 (or 8 + 2) ds_read_b128 feed 24 (12) v_mfma_f32_32x32x16_bf16;
//   * 32-k stages, two LDS buffers (2 x 64 KB / 2 x 48 KB): the next stage is copied global -> LDS by the DMA path
//     (global_load_lds_dwordx4: no staging VGPRs, no ds_write pass) while the current one is multiplied;
//   * LDS image: rows of 64 B (4 chunks of 16 B = 8 bf16), chunk' = chunk ^ ((row >> 2) & 3): the 16 lanes of every ds_read_b128
//     group hit 16 distinct bank slots.  The DMA writes LDS lane-linearly, so the swizzle is applied to the SOURCE address;
//   * same products, same k order inside a 16-k step and across steps as the 128 x 128 tile: bit-identical results.
// Ping-pong schedule (MI355X_MICROARCH.md "Two waves per SIMD"): the workgroup's two waves on a SIMD share that SIMD's matrix pipe,
// so if all eight waves ran the same phase (barrier -> LDS reads -> 48 MFMAs) the pipe would idle through every read / DMA-issue
// phase (the lock-step form this tile replaced: DESIGN_HISTORY.md).  The wave halves (waves 0-3 = rows 0-127, waves 4-7 = rows
// 128-255; one of each per SIMD) run half a 16-k step apart: while one half issues its 24 MFMAs the other fetches its next
// fragments from LDS and issues its share of the next stage's DMA; an s_barrier separates the phases (4 per 32-k stage).  Per stage s:
//     phase 4s     A: read fragments (s, k-half 0)                              B: multiply (s-1, 1)
//     phase 4s+1   A: multiply (s, 0) + DMA share of stage s+1                  B: read (s, 0)
//     phase 4s+2   A: read (s, 1), own DMA pieces landed                        B: multiply (s, 0) + DMA share of s+1
//     phase 4s+3   A: multiply (s, 1)                                           B: read (s, 1), own DMA pieces landed
// Buffer (s+1)&1 is rewritten from phase 4s+1 on: its last readers were phases 4s-2 (A) and 4s-1 (B); it is first read in 4s+4.
// (The accumulator clear, the DMA source offsets, the C-store epilogue and the queue loop of the XCD-filtered forms are spelled out in
// every kernel that has them: as shared inline helpers each of them changed the register allocation or the instruction count of a tile.)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool v_is_magic(float v) { return v == 1.2345678e33f; }   // (debug switch of tools/gemm_bench.py: keeps the accumulators live)
__device__ __forceinline__ int qswz(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// (sched_barrier: MFMAs are register-only instructions, a "memory" clobber alone lets the scheduler carry them across the barrier
// into the other phase -- which is exactly what the phases exist to prevent)
__device__ __forceinline__ void pp_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void pp_barrier_vm() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

#ifdef CTCN_GEMM_STATS
// development (tools/mb_gemm_pp.hip): per barrier site of the main loop, the cycles a wave spends before it reaches the barrier (its phase's own
// work) and inside it (waiting for the other waves), summed over the stages of one tile: waves 0 and 4 of blocks 0 and 1000
__device__ long long *g_gemm_stats;
#define PPB_SITE(i, vm)                                                                                                   \
  do {                                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    if (vm) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    const long long ta_ = clock64();                                                                                      \
    asm volatile("s_barrier" ::: "memory");                                                                               \
    const long long tb_ = clock64();                                                                                      \
    gs_work[i] += ta_ - gs_prev; gs_wait[i] += tb_ - ta_; gs_prev = tb_;                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  } while (0)
#define PPB(i) PPB_SITE(i, false)
#define PPB_VM(i) PPB_SITE(i, true)
#else
#define PPB(i) pp_barrier()
#define PPB_VM(i) pp_barrier_vm()
#endif
// one 256 x (128 * WNT) output tile (tile number `bid`, row-major over tiles_m x tiles_n) in the ping-pong schedule
// NP = 3: the bf16x3 products (al*bh, ah*bl, ah*bh); NP = 1 (option "gemm_bf16_single"): ah*bh only -- plain bf16 operands, f32 accumulate: the lo
// planes are neither copied nor read (the LDS image keeps its layout, the lo halves of a stage stay unused)
template <int WNT, int NP = 3>
__device__ __forceinline__ void planes256pp_tile(unsigned char *qsm, int bid, int M, int N, int Kp, const unsigned short *__restrict__ Ah,
                                                 const unsigned short *__restrict__ Al, const unsigned short *__restrict__ Bh,
                                                 const unsigned short *__restrict__ Bl, float *__restrict__ C, int ldc, float beta, int tiles_n, int dbg) {
  constexpr int TBM = 256, TBN = 128 * WNT;
  constexpr int A_BYTES = TBM * 64, B_BYTES = TBN * 64;
  constexpr int STAGE = 2 * A_BYTES + 2 * B_BYTES;
  constexpr int IA = TBM * 4 / 512, IB = TBN * 4 / 512;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * TBM, n0 = tn * TBN;
#ifdef CTCN_GEMM_STATS
  const long long gs_entry = clock64();
#endif

  f32x16 acc[4][WNT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // DMA source offsets (elements) of this lane: LDS position p = (inst * 8 + wave) * 64 + lane -> row p >> 2, swizzled chunk p & 3
  unsigned offA[IA], offB[IB];
#pragma unroll
  for (int i = 0; i < IA; ++i) {
    const int p = (i * 8 + wave) * 64 + lane, row = p >> 2, chunk = (p & 3) ^ ((row >> 2) & 3);
    offA[i] = (unsigned)min(m0 + row, M - 1) * (unsigned)Kp + chunk * 8;
  }
#pragma unroll
  for (int i = 0; i < IB; ++i) {
    const int p = (i * 8 + wave) * 64 + lane, row = p >> 2, chunk = (p & 3) ^ ((row >> 2) & 3);
    offB[i] = (unsigned)min(n0 + row, N - 1) * (unsigned)Kp + chunk * 8;
  }
  typedef const __attribute__((address_space(1))) void *gptr_t;
  typedef __attribute__((address_space(3))) void *lptr_t;
  auto issue = [&](int k0, int buf) {
    unsigned char *sb = qsm + buf * STAGE;
#pragma unroll
    for (int i = 0; i < IA; ++i) {
      const int dst = (i * 8 + wave) * 1024;
      __builtin_amdgcn_global_load_lds((gptr_t)(Ah + offA[i] + k0), (lptr_t)(sb + dst), 16, 0, 0);
      if constexpr (NP == 3) __builtin_amdgcn_global_load_lds((gptr_t)(Al + offA[i] + k0), (lptr_t)(sb + A_BYTES + dst), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      const int dst = (i * 8 + wave) * 1024;
      __builtin_amdgcn_global_load_lds((gptr_t)(Bh + offB[i] + k0), (lptr_t)(sb + 2 * A_BYTES + dst), 16, 0, 0);
      if constexpr (NP == 3) __builtin_amdgcn_global_load_lds((gptr_t)(Bl + offB[i] + k0), (lptr_t)(sb + 2 * A_BYTES + B_BYTES + dst), 16, 0, 0);
    }
  };
  const int nst = Kp / 32;
  const int ml = lane & 31, g = lane >> 5;
  bf16x8_t ah[4], al[4], bh[WNT], bl[WNT];
  // LDS byte offsets of this lane's fragments inside a stage, per 16-k half (loop-invariant)
  int oa[2][4], ob[2][WNT];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) oa[ks][i] = qswz(wm * 128 + i * 32 + ml, ks * 2 + g);
#pragma unroll
    for (int j = 0; j < WNT; ++j) ob[ks][j] = 2 * A_BYTES + qswz(wn * 32 * WNT + j * 32 + ml, ks * 2 + g);
  }
  auto load_frags = [&](int stage, int ks) {
    const unsigned char *sb = qsm + (stage & 1) * STAGE;
#pragma unroll
    for (int j = 0; j < WNT; ++j) {
      bh[j] = *reinterpret_cast<const bf16x8_t *>(sb + ob[ks][j]);
      if constexpr (NP == 3) bl[j] = *reinterpret_cast<const bf16x8_t *>(sb + B_BYTES + ob[ks][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ah[i] = *reinterpret_cast<const bf16x8_t *>(sb + oa[ks][i]);
      if constexpr (NP == 3) al[i] = *reinterpret_cast<const bf16x8_t *>(sb + A_BYTES + oa[ks][i]);
    }
  };
  // one DMA piece (1 KB) of this wave's share of a stage: n = 0 .. NPIECE - 1
  auto issue_piece = [&](int n, int k0, int buf) {
    unsigned char *sb = qsm + buf * STAGE;
    if constexpr (NP == 3) {
      if (n < 2 * IA) {
        const int i = n >> 1, dst = (i * 8 + wave) * 1024;
        if (n & 1) __builtin_amdgcn_global_load_lds((gptr_t)(Al + offA[i] + k0), (lptr_t)(sb + A_BYTES + dst), 16, 0, 0);
        else __builtin_amdgcn_global_load_lds((gptr_t)(Ah + offA[i] + k0), (lptr_t)(sb + dst), 16, 0, 0);
      } else {
        const int m = n - 2 * IA, i = m >> 1, dst = (i * 8 + wave) * 1024;
        if (m & 1) __builtin_amdgcn_global_load_lds((gptr_t)(Bl + offB[i] + k0), (lptr_t)(sb + 2 * A_BYTES + B_BYTES + dst), 16, 0, 0);
        else __builtin_amdgcn_global_load_lds((gptr_t)(Bh + offB[i] + k0), (lptr_t)(sb + 2 * A_BYTES + dst), 16, 0, 0);
      }
    } else {
      if (n < IA) __builtin_amdgcn_global_load_lds((gptr_t)(Ah + offA[n] + k0), (lptr_t)(sb + (n * 8 + wave) * 1024), 16, 0, 0);
      else __builtin_amdgcn_global_load_lds((gptr_t)(Bh + offB[n - IA] + k0), (lptr_t)(sb + 2 * A_BYTES + ((n - IA) * 8 + wave) * 1024), 16, 0, 0);
    }
  };
  constexpr int NPIECE = NP == 3 ? 2 * IA + 2 * IB : IA + IB, NMM = 4 * WNT;
  // 24 (12) MFMAs -- NP = 1: 8 (4) --; with `dma` the wave's DMA pieces of the next stage are issued between them (an LDS-DMA instruction costs the
  // issuing wave ~60 cycles among bare MFMAs and 100-185 inside a read phase: MI355X_MICROARCH.md), one piece per (i, j) tile
  auto multiply = [&](auto dma, int k0, int buf) {
#pragma unroll
    for (int t = 0; t < NP; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WNT; ++j) {
          // term order per accumulator: al*bh, ah*bl, ah*bh (small terms first) -- as in the other plane tiles
          if (NP == 3 && t == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          else if (NP == 3 && t == 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          const int n = t * NMM + i * WNT + j;                 // running MFMA number; pieces after MFMAs 1, 3, 5, ... (NP = 1: after every MFMA)
          const int pc = NP == 3 ? ((n & 1) ? (n >> 1) : NPIECE) : n;
          if (pc < NPIECE) {
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(dma)::value) issue_piece(pc, k0, buf);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
  };
  // ONE instruction stream for both halves -- read (s,0) | multiply | read (s,1) | multiply, a barrier after each step -- which
  // half B enters one barrier late: at every moment one half multiplies while the other reads
  issue(0, 0);
  pp_barrier_vm();                              // stage 0 landed
  if (wm == 1) pp_barrier();
  constexpr std::integral_constant<bool, true> with_dma{};
  constexpr std::integral_constant<bool, false> no_dma{};
#ifdef CTCN_GEMM_STATS
  long long gs_work[4] = {0, 0, 0, 0}, gs_wait[4] = {0, 0, 0, 0};
  const long long gs_t0 = clock64();
  long long gs_prev = gs_t0;
#endif
  for (int s = 0; s + 1 < nst; ++s) {
    load_frags(s, 0);
    PPB(0);
    multiply(with_dma, (s + 1) * 32, (s + 1) & 1);          // + DMA share of stage s + 1 (buffer last read >= 2 steps ago by either half)
    PPB(1);
    load_frags(s, 1);
    if (dbg & 8) PPB(2); else PPB_VM(2);                    // own DMA pieces of stage s + 1 landed  (dbg 8: timing experiment, wrong results)
    multiply(no_dma, 0, 0);
    PPB(3);
  }
#ifdef CTCN_GEMM_STATS
  if (lane == 0 && (wave & 3) == 0 && (blockIdx.x == 0 || blockIdx.x == 1000) && g_gemm_stats) {
    long long *o = g_gemm_stats + ((blockIdx.x ? 2 : 0) + (wave >> 2)) * 16;
    for (int i = 0; i < 4; ++i) { o[i] = gs_work[i]; o[4 + i] = gs_wait[i]; }
    o[8] = clock64() - gs_t0; o[9] = nst - 1;
  }
#endif
  load_frags(nst - 1, 0);
  pp_barrier();
  multiply(no_dma, 0, 0);
  pp_barrier();
  load_frags(nst - 1, 1);
  pp_barrier();
  multiply(no_dma, 0, 0);
  pp_barrier();
  if (wm == 0) pp_barrier();                    // (half B's last multiply)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j) {
      const int col = n0 + wn * 32 * WNT + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 128 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < M && col < N && (!(dbg & 1) || v_is_magic(acc[i][j][e]))) {
          float v = acc[i][j][e];
          float *p = C + (size_t)row * ldc + col;
          if (beta != 0.0f) v += beta * *p;
          if (dbg & 4) __builtin_nontemporal_store(v, p); else *p = v;
        }
      }
    }
#ifdef CTCN_GEMM_STATS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0 && (wave & 3) == 0 && (blockIdx.x == 0 || blockIdx.x == 1000) && g_gemm_stats)
    g_gemm_stats[((blockIdx.x ? 2 : 0) + (wave >> 2)) * 16 + 10] = clock64() - gs_entry;
#endif
}

template <int WNT, int NP = 3>
__global__ __launch_bounds__(512) void gemm_planes_nt256pp_kernel(int M, int N, int Kp, const unsigned short *__restrict__ Ah,
                                                                  const unsigned short *__restrict__ Al, const unsigned short *__restrict__ Bh,
                                                                  const unsigned short *__restrict__ Bl, float *__restrict__ C, int ldc, float beta,
                                                                  int tiles_m, int tiles_n, int dbg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
  const int bid = xcd_band_tile(blockIdx.x, tiles_m * tiles_n);
  planes256pp_tile<WNT, NP>(qsm, bid, M, N, Kp, Ah, Al, Bh, Bl, C, ldc, beta, tiles_n, dbg);
}

// XCD-filtered form for a side stream next to a persistent recurrence (see gemm_planes_nt_queue_kernel): workgroups off `xcd_allow`
// leave, the others take tiles from an atomic queue.  The same tile code: bit-identical results.
template <int WNT, int NP = 3>
__global__ __launch_bounds__(512) void gemm_planes_nt256pp_queue_kernel(int M, int N, int Kp, const unsigned short *__restrict__ Ah,
                                                                        const unsigned short *__restrict__ Al, const unsigned short *__restrict__ Bh,
                                                                        const unsigned short *__restrict__ Bl, float *__restrict__ C, int ldc, float beta,
                                                                        int tiles_m, int tiles_n, unsigned xcd_allow, unsigned *__restrict__ queue) {
  extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
  __shared__ int s_item;
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  if (!((xcd_allow >> (x & 15)) & 1u)) return;
  const int nt = tiles_m * tiles_n;
  for (;;) {
    if (threadIdx.x == 0) s_item = (int)atomicAdd(queue, 1u);
    __syncthreads();
    const int item = s_item;
    if (item >= nt) return;
    planes256pp_tile<WNT, NP>(qsm, item, M, N, Kp, Ah, Al, Bh, Bl, C, ldc, beta, tiles_n, 0);
    __syncthreads();
  }
}

// The float32-A tile: the same tile with the A operand taken straight from the float32 matrix (row-major, k contiguous) and split
// into hi / lo bf16 while it is staged: no plane pass over A (for da = 25 600 x 2 560 that pass moves 524 MB, 91 us -- a third of the
// product's own time).  B (the weights) still comes pre-split through the DMA path.  The ping-pong schedule of
// gemm_planes_nt256pp_kernel (one instruction stream, half B one barrier behind):
//     read (s, k-half 0) | multiply + the wave's DMA pieces of B(s+1) | read (s, 1), convert + store A(s+1), own DMA landed |
//     multiply + global loads of A(s+2)
// A thread stages its own 16 floats of a row of A: loaded during the second multiply of stage s-1, split into hi / lo (the same
// split_bf16 as everywhere: identical planes) and written into the other LDS buffer during the second read phase of stage s, three
// phases later.
// NP = 1 (option "gemm_bf16_single"): ah*bh only -- A rounded to bf16 as it is staged, the lo plane of B neither copied nor read.
template <int WNT, int NP = 3>
__global__ __launch_bounds__(512) void gemm_planes_nt256pp_af32_kernel(int M, int N, int K, int Kp, const float *__restrict__ A, int lda,
                                                                       const unsigned short *__restrict__ Bh, const unsigned short *__restrict__ Bl,
                                                                       float *__restrict__ C, int ldc, float beta, int tiles_m, int tiles_n) {
  constexpr int TBM = 256, TBN = 128 * WNT;
  constexpr int A_BYTES = TBM * 64, B_BYTES = TBN * 64;
  constexpr int STAGE = 2 * A_BYTES + 2 * B_BYTES;
  constexpr int IB = TBN * 4 / 512;
  extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int bid = xcd_band_tile(blockIdx.x, tiles_m * tiles_n);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * TBM, n0 = tn * TBN;

  f32x16 acc[4][WNT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  unsigned offB[IB];
#pragma unroll
  for (int i = 0; i < IB; ++i) {
    const int p = (i * 8 + wave) * 64 + lane, row = p >> 2, chunk = (p & 3) ^ ((row >> 2) & 3);
    offB[i] = (unsigned)min(n0 + row, N - 1) * (unsigned)Kp + chunk * 8;
  }
  typedef const __attribute__((address_space(1))) void *gptr_t;
  typedef __attribute__((address_space(3))) void *lptr_t;
  constexpr int NBP = NP == 3 ? 2 * IB : IB;                   // DMA pieces of B per wave and stage
  auto issue_b_piece = [&](int n, int k0, int buf) {            // n = 0 .. NBP-1
    unsigned char *sb = qsm + buf * STAGE + 2 * A_BYTES;
    if constexpr (NP == 3) {
      const int i = n >> 1, dst = (i * 8 + wave) * 1024;
      if (n & 1) __builtin_amdgcn_global_load_lds((gptr_t)(Bl + offB[i] + k0), (lptr_t)(sb + B_BYTES + dst), 16, 0, 0);
      else __builtin_amdgcn_global_load_lds((gptr_t)(Bh + offB[i] + k0), (lptr_t)(sb + dst), 16, 0, 0);
    } else {
      __builtin_amdgcn_global_load_lds((gptr_t)(Bh + offB[n] + k0), (lptr_t)(sb + (n * 8 + wave) * 1024), 16, 0, 0);
    }
  };
  // A staging of this thread: the 16-B bf16 chunk `ach` (8 consecutive k = two float4) of rows arow0 and 128 + arow0 of the tile -- four
  // lanes per row, so that the eight lanes of a ds_write_b128 group cover two whole rows = 128 contiguous bytes (two lanes per row, 32 B
  // apart, hit every bank twice: 22 % of the kernel's LDS cycles were write conflicts).  The loads are bare, from clamped addresses: a
  // select on the loaded value made the wave wait for every load where it is issued, i.e. inside the multiply phase.  K % 4 == 0: a
  // piece is inside the matrix or outside it as a whole, and the ones outside are zeroed when they are split.
  const int arow0 = tid >> 2, ach = tid & 3;
  // aw[2 * r + h]: row r (arow0 / 128 + arow0) of the tile, floats 4 h .. 4 h + 3 of the thread's eight.  The loads are issued by hand (uniform
  // base = first row of the tile + k0 in SGPRs, this lane's row / column as a 32-bit offset: no address arithmetic per stage) and waited for
  // by hand (WAIT_A): with loads of two stages in flight hipcc puts s_waitcnt vmcnt(0) in front of the first use of the older ones, i.e.
  // waits for the loads it has just issued
  u32x4 aw[4];
  const float *atile = A + (size_t)m0 * lda;
  const unsigned arel[2] = {(unsigned)min(arow0, M - 1 - m0) * (unsigned)lda, (unsigned)min(128 + arow0, M - 1 - m0) * (unsigned)lda};
  auto load_a_piece = [&](int q, int k0) {                     // q = 2 * row + half
    // ONE asm statement per piece (an if / else around two of them lets the compiler merge the two "results" with register copies behind the
    // branch -- of registers whose load is still in flight).  The stage that holds the end of K is clamped per lane (the split zeroes what
    // lies beyond K); every other stage adds k0 on the scalar side
    const int c = 8 * ach + 4 * (q & 1);
    const bool whole = k0 + 32 <= K;
    const float *sbase = atile + (whole ? k0 : 0);
    const unsigned voff = (arel[q >> 1] + (unsigned)(whole ? c : min(k0 + c, K - 4))) * 4u;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(aw[q]) : "v"(voff), "s"(sbase) : "memory");
  };
#ifdef CTCN_GEMM_NOVM      // (timing experiment of tools/mb_gemm_pp.hip: wrong results)
#define WAIT_A(N, r) asm volatile("" : "+v"(aw[2 * (r)]), "+v"(aw[2 * (r) + 1])::"memory")
#else
#define WAIT_A(N, r) asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(aw[2 * (r)]), "+v"(aw[2 * (r) + 1])::"memory")
#endif
  // two neighbours at a time: hi = bf16(x) of both in one v_cvt_pk_bf16_f32, lo = bf16(x - hi) likewise (the split_bf16 values)
  auto split_pair = [](float a, float b, unsigned &hw, unsigned &lw) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    hw = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
    const f32x2_t r = {a - __uint_as_float(hw << 16), b - __uint_as_float(hw & 0xffff0000u)};
    lw = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_t));
  };
  // half h of row r (four consecutive floats) of the stage that starts at k0, in place: {x0, x1, x2, x3} -> {hi01, hi23, lo01, lo23}
  auto convert_half = [&](int r, int h, int k0) {
    u32x4 w = aw[2 * r + h];
    if (k0 + 32 > K && k0 + 8 * ach + 4 * h >= K) w = (u32x4){0u, 0u, 0u, 0u};          // (K % 4 == 0: a 16-B piece is inside or outside as a whole)
    unsigned h0, l0, h1, l1;
    if constexpr (NP == 3) {
      split_pair(__uint_as_float(w[0]), __uint_as_float(w[1]), h0, l0);
      split_pair(__uint_as_float(w[2]), __uint_as_float(w[3]), h1, l1);
    } else {
      typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
      typedef float f32x2_t __attribute__((ext_vector_type(2)));
      h0 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){__uint_as_float(w[0]), __uint_as_float(w[1])}, bf16x2_t));
      h1 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){__uint_as_float(w[2]), __uint_as_float(w[3])}, bf16x2_t));
      l0 = l1 = 0u;
    }
    aw[2 * r + h] = (u32x4){h0, h1, l0, l1};
  };
  // the converted row r -> its 16-B chunk of either plane, as two 8-B halves each (straight from the register pairs convert_half left; four
  // lanes per row: a row's 64 B are contiguous)
  auto store_a_row = [&](int r, int buf) {
    unsigned char *sb = qsm + buf * STAGE + qswz(arow0 + 128 * r, ach);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<u32x2 *>(sb + 8 * h) = (u32x2){aw[2 * r + h][0], aw[2 * r + h][1]};
      if constexpr (NP == 3) *reinterpret_cast<u32x2 *>(sb + A_BYTES + 8 * h) = (u32x2){aw[2 * r + h][2], aw[2 * r + h][3]};
    }
  };
  const int nst = Kp / 32;
  const int ml = lane & 31, g = lane >> 5;
  bf16x8_t ah[4], al[4], bh[WNT], bl[WNT];
  int oa[2][4], ob[2][WNT];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) oa[ks][i] = qswz(wm * 128 + i * 32 + ml, ks * 2 + g);
#pragma unroll
    for (int j = 0; j < WNT; ++j) ob[ks][j] = 2 * A_BYTES + qswz(wn * 32 * WNT + j * 32 + ml, ks * 2 + g);
  }
  auto load_frags = [&](int stage, int ks) {
    const unsigned char *sb = qsm + (stage & 1) * STAGE;
#pragma unroll
    for (int j = 0; j < WNT; ++j) {
      bh[j] = *reinterpret_cast<const bf16x8_t *>(sb + ob[ks][j]);
      if constexpr (NP == 3) bl[j] = *reinterpret_cast<const bf16x8_t *>(sb + B_BYTES + ob[ks][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ah[i] = *reinterpret_cast<const bf16x8_t *>(sb + oa[ks][i]);
      if constexpr (NP == 3) al[i] = *reinterpret_cast<const bf16x8_t *>(sb + A_BYTES + oa[ks][i]);
    }
  };
  constexpr int NMM = 4 * WNT;
  // One multiply phase: 3 * NMM MFMAs with the wave's other work of the stage between them, one item behind an MFMA:
  //   WHICH 1 (first multiply of stage s):  DMA pieces of B(s+1) | split of A(s+1) row 1 (loaded three phases ago)
  //   WHICH 2 (second multiply):            split of A(s+2) row 0 (loaded three phases ago)
  // HAS1: stage s + 1 exists, HAS2: stage s + 2 exists.  The float32 -> hi / lo split (12 VALU instructions per four floats) sits in the
  // shadow of the wave's OWN MFMAs, ~5 cycles per instruction: in the read phases, next to the other half's MFMAs, the same instructions cost
  // 15-20 cycles each (as one block of both rows that phase was 1 100-1 400 cycles long against the 430-500 of the MFMAs it is meant to hide
  // behind; one row per read phase: 800 -- tools/mb_gemm_pp.hip).  The A loads leave from the READ phases (row 0 of A(s+2) in the first one of
  // stage s, row 1 in the second, each right behind the ds_write that freed its registers).  In flight, oldest first (loads and DMA pieces
  // return in order), when the split starts: first multiply: A(s+1) row 1 (2 loads), A(s+2) row 0 (2, HAS2), this phase's 2 IB DMA pieces;
  // second multiply: A(s+2) row 1 (2) -- row 0 and the DMA pieces were waited for in front of the barrier before it
  auto multiply = [&](auto which, auto has1, auto has2, int s) {
    constexpr int WHICH = decltype(which)::value;
    constexpr bool HAS1 = decltype(has1)::value, HAS2 = decltype(has2)::value;
    constexpr int CV0 = NP * NMM - 3;                          // the two splits go behind the third- and second-to-last MFMA (the loads have had the longest time)
    static_assert(NBP <= CV0, "DMA slots and split slots of a multiply phase overlap");
#pragma unroll
    for (int t = 0; t < NP; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WNT; ++j) {
          if (NP == 3 && t == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);   // small terms first
          else if (NP == 3 && t == 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          const int n = t * NMM + i * WNT + j;
          if (n < NBP || n == CV0 || n == CV0 + 1) {
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (WHICH == 1) {
              if (HAS1 && n < NBP) issue_b_piece(n, (s + 1) * 32, (s + 1) & 1);
              if (HAS1 && n == CV0) {          // A(s+1) row 1 has landed: what may stay in flight is A(s+2) row 0 (2 loads, HAS2) + this phase's NBP pieces
                constexpr int OUT = (HAS2 ? 2 : 0) + NBP;
                if constexpr (OUT == 1) WAIT_A(1, 1); else if constexpr (OUT == 2) WAIT_A(2, 1); else if constexpr (OUT == 3) WAIT_A(3, 1);
                else if constexpr (OUT == 4) WAIT_A(4, 1); else { static_assert(OUT <= 4 || OUT == 6, "vmcnt literal"); WAIT_A(6, 1); }
              }
              if (HAS1 && n >= CV0) convert_half(1, n - CV0, (s + 1) * 32);
            } else {
              if (HAS2 && n == CV0) WAIT_A(2, 0);
              if (HAS2 && n >= CV0) convert_half(0, n - CV0, (s + 2) * 32);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
  };
  constexpr std::integral_constant<int, 1> first{};
  constexpr std::integral_constant<int, 2> second{};
  constexpr std::integral_constant<bool, true> yes{};
  constexpr std::integral_constant<bool, false> no{};
  // prologue: stage 0 into buffer 0 (A through the registers, B by DMA), all of A(1) into the registers
#pragma unroll
  for (int q = 0; q < 4; ++q) aw[q] = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
  for (int q = 0; q < 4; ++q) load_a_piece(q, 0);
#pragma unroll
  for (int n = 0; n < NBP; ++n) issue_b_piece(n, 0, 0);
  WAIT_A(0, 0); WAIT_A(0, 1);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    convert_half(r, 0, 0); convert_half(r, 1, 0);
    store_a_row(r, 0);
  }
  if (nst > 1) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // (the ds_writes have read aw)
#pragma unroll
    for (int q = 0; q < 4; ++q) load_a_piece(q, 32);
    WAIT_A(2, 0);
    convert_half(0, 0, 32); convert_half(0, 1, 32);           // row 0 of A(1): the first read phase stores it; row 1 is split in the first multiply
  }
  pp_barrier_vm();
  if (wm == 1) pp_barrier();
#ifdef CTCN_GEMM_STATS
  long long gs_work[4] = {0, 0, 0, 0}, gs_wait[4] = {0, 0, 0, 0};
  const long long gs_t0 = clock64();
  long long gs_prev = gs_t0;
#endif
  auto stage = [&](int s, auto has1, auto has2) {
    constexpr bool HAS1 = decltype(has1)::value, HAS2 = decltype(has2)::value;
    load_frags(s, 0);
    if constexpr (HAS1) store_a_row(0, (s + 1) & 1);          // A(s+1) row 0 (split in the previous multiply phase) -> the other buffer (last read two phases ago)
    if constexpr (HAS2) {                                     // its registers take A(s+2) row 0 (the ds_write above has read them at issue; the load returns hundreds of cycles later)
      __builtin_amdgcn_sched_barrier(0);
      load_a_piece(0, (s + 2) * 32); load_a_piece(1, (s + 2) * 32);
    }
    PPB(0);
    multiply(first, has1, has2, s);
    PPB(1);
    load_frags(s, 1);
    if constexpr (HAS1) store_a_row(1, (s + 1) & 1);          // A(s+1) row 1 (split in the multiply phase just before)
    if constexpr (HAS2) {
      __builtin_amdgcn_sched_barrier(0);
      load_a_piece(2, (s + 2) * 32); load_a_piece(3, (s + 2) * 32);
    }
    // this wave's DMA pieces of B(s+1) have landed (and A(s+2) row 0, older; the two loads of row 1, just issued, stay in flight)
#ifdef CTCN_GEMM_STATS
    PPB_VM(2);
#else
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HAS2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#endif
    multiply(second, has1, has2, s);
    PPB(3);
  };
  int s = 0;
  for (; s + 2 < nst; ++s) stage(s, yes, yes);
#ifdef CTCN_GEMM_STATS
  if (lane == 0 && (wave & 3) == 0 && (blockIdx.x == 0 || blockIdx.x == 1000) && g_gemm_stats) {
    long long *o = g_gemm_stats + ((blockIdx.x ? 2 : 0) + (wave >> 2)) * 16;
    for (int i = 0; i < 4; ++i) { o[i] = gs_work[i]; o[4 + i] = gs_wait[i]; }
    o[8] = clock64() - gs_t0; o[9] = nst - 2; o[10] = 0;
  }
#endif
  if (s + 1 < nst) { stage(s, yes, no); ++s; }
  stage(s, no, no);
  if (wm == 0) pp_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j) {
      const int col = n0 + wn * 32 * WNT + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 128 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < M && col < N) {
          float v = acc[i][j][e];
          float *p = C + (size_t)row * ldc + col;
          if (beta != 0.0f) v += beta * *p;
          *p = v;
        }
      }
    }
}

// The float32-A tile at 256 x 320, for the dx product of a 320-unit bidirectional layer (N = 640 = 2 x 320: 200 tiles, one round on 256 CUs,
// where the 256 x 128 tile above takes 500 tiles in two rounds and its 12-MFMA multiply phases cannot cover the other half's read phase).
// The schedule, the A staging and the LDS image of gemm_planes_nt256pp_af32_kernel, a kernel of its own so that that one's code stays as it is:
//   * the eight waves as 4 (M) x 2 (N): a wave owns 64 x 160 outputs = 2 x 5 MFMA tiles (160 accumulator registers); per 16-k half-stage
//     4 + 10 ds_read_b128 feed 30 MFMAs.  Waves 0-3 hold rows 0-127 and waves 4-7 rows 128-255: the ping-pong halves, one of each per SIMD;
//   * a stage is A hi / lo 2 x 16 KB + B hi / lo 2 x 20 KB = 72 KB, two buffers 144 KB;
//   * B by DMA: 2 planes x 20 sixteen-row pieces of 1 KB per stage, five per wave -- piece n of wave w is number 8 n + w: plane w & 1,
//     rows 16 (4 n + (w >> 1)) onwards.  N % 320 == 0 (the host's condition): no row of B is clamped.
// Per accumulator and 16-k step the products al*bh, ah*bl, ah*bh in that order, on the split_bf16 planes, k ascending: bit-identical to the
// other plane tiles.  bf16x3 only (option "gemm_bf16_single" keeps the 256 x 128 tile).
// gfx950, hipcc -O3 (-Rpass-analysis=kernel-resource-usage): 256 VGPRs of the unified file (160 of them accumulators, no AGPRs), 50 SGPRs, no
// scratch, 147 456 B of dynamic LDS.  Every register is taken: the B pieces are issued by hand from a scalar base and the epilogue recomputes
// its lane number for that reason (each cost 1-3 spilled registers otherwise); check the remark after any edit.
__global__ __launch_bounds__(512) void gemm_af32_n320pp_kernel(int M, int N, int K, int Kp, const float *__restrict__ A, int lda,
                                                               const unsigned short *__restrict__ Bh, const unsigned short *__restrict__ Bl,
                                                               float *__restrict__ C, int ldc, float beta, int tiles_m, int tiles_n) {
  constexpr int TBM = 256, TBN = 320, WI = 2, WJ = 5;
  constexpr int A_BYTES = TBM * 64, B_BYTES = TBN * 64;
  constexpr int STAGE = 2 * A_BYTES + 2 * B_BYTES;
  constexpr int NBP = 2 * TBN / 16 / 8;                        // DMA pieces of B per wave and stage: 5
  extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int bid = xcd_band_tile(blockIdx.x, tiles_m * tiles_n);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * TBM, n0 = tn * TBN;

  f32x16 acc[WI][WJ];
#pragma unroll
  for (int i = 0; i < WI; ++i)
#pragma unroll
    for (int j = 0; j < WJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // DMA source of this lane in the wave's first piece: LDS position lane -> row lane >> 2 of the piece, swizzled chunk (the piece's first row is
  // a multiple of 16: the swizzle term is the lane's own); the wave's further pieces lie 64 rows apart
  const unsigned short *const bplane = (wave & 1) ? Bl : Bh;
  const int bdst = 2 * A_BYTES + (wave & 1) * B_BYTES + (wave >> 1) * 1024;
  const unsigned offB = ((unsigned)(n0 + (wave >> 1) * 16 + (lane >> 2)) * (unsigned)Kp + (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 8)) * 2u;   // bytes
  typedef __attribute__((address_space(3))) unsigned char *lds_u8_t;
  auto issue_b_piece = [&](int n, int k0, int buf) {            // n = 0 .. NBP-1
    // issued by hand: the piece's base in a scalar pair + the lane's 32-bit offset, the LDS address in M0, written in the statement that reads
    // it (the kernel has no other user of M0).  The builtin on a pointer forms per-lane 64-bit addresses that advance with k0: four more
    // registers than the kernel has.  The waits for the pieces are the kernel's own (WAIT_A, the vmcnt in front of the third barrier)
    const unsigned short *sbase = bplane + (size_t)n * 64 * Kp + k0;
    const unsigned dst = (unsigned)(uintptr_t)(lds_u8_t)(qsm + buf * STAGE + bdst + n * 4096);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(dst), "v"(offB), "s"(sbase) : "memory");
  };
  // A staging: as in gemm_planes_nt256pp_af32_kernel (the comments there) -- the 16-B bf16 chunk `ach` of rows arow0 and 128 + arow0 of the tile
  const int arow0 = tid >> 2, ach = tid & 3;
  u32x4 aw[4];
  const float *atile = A + (size_t)m0 * lda;
  const unsigned arel[2] = {(unsigned)min(arow0, M - 1 - m0) * (unsigned)lda, (unsigned)min(128 + arow0, M - 1 - m0) * (unsigned)lda};
  auto load_a_piece = [&](int q, int k0) {                     // q = 2 * row + half
    const int c = 8 * ach + 4 * (q & 1);
    const bool whole = k0 + 32 <= K;
    const float *sbase = atile + (whole ? k0 : 0);
    const unsigned voff = (arel[q >> 1] + (unsigned)(whole ? c : min(k0 + c, K - 4))) * 4u;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(aw[q]) : "v"(voff), "s"(sbase) : "memory");
  };
  auto split_pair = [](float a, float b, unsigned &hw, unsigned &lw) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    hw = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
    const f32x2_t r = {a - __uint_as_float(hw << 16), b - __uint_as_float(hw & 0xffff0000u)};
    lw = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_t));
  };
  auto convert_half = [&](int r, int h, int k0) {
    u32x4 w = aw[2 * r + h];
    if (k0 + 32 > K && k0 + 8 * ach + 4 * h >= K) w = (u32x4){0u, 0u, 0u, 0u};          // (K % 4 == 0: a 16-B piece is inside or outside as a whole)
    unsigned h0, l0, h1, l1;
    split_pair(__uint_as_float(w[0]), __uint_as_float(w[1]), h0, l0);
    split_pair(__uint_as_float(w[2]), __uint_as_float(w[3]), h1, l1);
    aw[2 * r + h] = (u32x4){h0, h1, l0, l1};
  };
  auto store_a_row = [&](int r, int buf) {
    unsigned char *sb = qsm + buf * STAGE + qswz(arow0 + 128 * r, ach);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<u32x2 *>(sb + 8 * h) = (u32x2){aw[2 * r + h][0], aw[2 * r + h][1]};
      *reinterpret_cast<u32x2 *>(sb + A_BYTES + 8 * h) = (u32x2){aw[2 * r + h][2], aw[2 * r + h][3]};
    }
  };
  const int nst = Kp / 32;
  const int ml = lane & 31, g = lane >> 5;
  bf16x8_t ah[WI], al[WI], bh[WJ], bl[WJ];
  // LDS offsets of this lane's fragments per 16-k half: the first MFMA tile's; the others lie 32 rows = 2 KB further each (the wave's first
  // row and 32 j are multiples of 16 rows, so the swizzle term is the lane's own)
  int oa[2], ob[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    oa[ks] = qswz(wm * 64 + ml, ks * 2 + g);
    ob[ks] = 2 * A_BYTES + qswz(wn * 160 + ml, ks * 2 + g);
  }
  auto load_frags = [&](int stage, int ks) {
    const unsigned char *sb = qsm + (stage & 1) * STAGE;
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      bh[j] = *reinterpret_cast<const bf16x8_t *>(sb + ob[ks] + j * 2048);
      bl[j] = *reinterpret_cast<const bf16x8_t *>(sb + B_BYTES + ob[ks] + j * 2048);
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      ah[i] = *reinterpret_cast<const bf16x8_t *>(sb + oa[ks] + i * 2048);
      al[i] = *reinterpret_cast<const bf16x8_t *>(sb + A_BYTES + oa[ks] + i * 2048);
    }
  };
  constexpr int NMM = WI * WJ;
  // One multiply phase: 30 MFMAs, the wave's other work of the stage one item behind an MFMA (WHICH, HAS1, HAS2 and the loads in flight: as in
  // gemm_planes_nt256pp_af32_kernel, with five DMA pieces)
  auto multiply = [&](auto which, auto has1, auto has2, int s) {
    constexpr int WHICH = decltype(which)::value;
    constexpr bool HAS1 = decltype(has1)::value, HAS2 = decltype(has2)::value;
    constexpr int CV0 = 3 * NMM - 3;
    static_assert(NBP <= CV0, "DMA slots and split slots of a multiply phase overlap");
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int i = 0; i < WI; ++i)
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
          if (t == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);   // small terms first
          else if (t == 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          const int n = t * NMM + i * WJ + j;
          if (n < NBP || n == CV0 || n == CV0 + 1) {
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (WHICH == 1) {
              if (HAS1 && n < NBP) issue_b_piece(n, (s + 1) * 32, (s + 1) & 1);
              if (HAS1 && n == CV0) {          // A(s+1) row 1 has landed: what may stay in flight is A(s+2) row 0 (2 loads, HAS2) + this phase's 5 pieces
                static_assert(NBP == 5, "vmcnt literals");
                if constexpr (HAS2) WAIT_A(7, 1); else WAIT_A(5, 1);
              }
              if (HAS1 && n >= CV0) convert_half(1, n - CV0, (s + 1) * 32);
            } else {
              if (HAS2 && n == CV0) WAIT_A(2, 0);
              if (HAS2 && n >= CV0) convert_half(0, n - CV0, (s + 2) * 32);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
  };
  constexpr std::integral_constant<int, 1> first{};
  constexpr std::integral_constant<int, 2> second{};
  constexpr std::integral_constant<bool, true> yes{};
  constexpr std::integral_constant<bool, false> no{};
  // prologue: stage 0 into buffer 0 (A through the registers, B by DMA), all of A(1) into the registers
#pragma unroll
  for (int q = 0; q < 4; ++q) aw[q] = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
  for (int q = 0; q < 4; ++q) load_a_piece(q, 0);
#pragma unroll
  for (int n = 0; n < NBP; ++n) issue_b_piece(n, 0, 0);
  WAIT_A(0, 0); WAIT_A(0, 1);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    convert_half(r, 0, 0); convert_half(r, 1, 0);
    store_a_row(r, 0);
  }
  if (nst > 1) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // (the ds_writes have read aw)
#pragma unroll
    for (int q = 0; q < 4; ++q) load_a_piece(q, 32);
    WAIT_A(2, 0);
    convert_half(0, 0, 32); convert_half(0, 1, 32);           // row 0 of A(1): the first read phase stores it; row 1 is split in the first multiply
  }
  pp_barrier_vm();
  if (wave >= 4) pp_barrier();                                // half B runs one barrier behind
#ifdef CTCN_GEMM_STATS
  long long gs_work[4] = {0, 0, 0, 0}, gs_wait[4] = {0, 0, 0, 0};
  const long long gs_t0 = clock64();
  long long gs_prev = gs_t0;
#endif
  auto stage = [&](int s, auto has1, auto has2) {
    constexpr bool HAS1 = decltype(has1)::value, HAS2 = decltype(has2)::value;
    load_frags(s, 0);
    if constexpr (HAS1) store_a_row(0, (s + 1) & 1);
    if constexpr (HAS2) {
      __builtin_amdgcn_sched_barrier(0);
      load_a_piece(0, (s + 2) * 32); load_a_piece(1, (s + 2) * 32);
    }
    PPB(0);
    multiply(first, has1, has2, s);
    PPB(1);
    load_frags(s, 1);
    if constexpr (HAS1) store_a_row(1, (s + 1) & 1);
    if constexpr (HAS2) {
      __builtin_amdgcn_sched_barrier(0);
      load_a_piece(2, (s + 2) * 32); load_a_piece(3, (s + 2) * 32);
    }
    // this wave's DMA pieces of B(s+1) have landed (and A(s+2) row 0, older; the two loads of row 1, just issued, stay in flight)
#ifdef CTCN_GEMM_STATS
    PPB_VM(2);
#else
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HAS2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#endif
    multiply(second, has1, has2, s);
    PPB(3);
  };
  int s = 0;
  for (; s + 2 < nst; ++s) stage(s, yes, yes);
#ifdef CTCN_GEMM_STATS
  if (lane == 0 && (wave & 3) == 0 && (blockIdx.x == 0 || blockIdx.x == 1000) && g_gemm_stats) {
    long long *o = g_gemm_stats + ((blockIdx.x ? 2 : 0) + (wave >> 2)) * 16;
    for (int i = 0; i < 4; ++i) { o[i] = gs_work[i]; o[4 + i] = gs_wait[i]; }
    o[8] = clock64() - gs_t0; o[9] = nst - 2; o[10] = 0;
  }
#endif
  if (s + 1 < nst) { stage(s, yes, no); ++s; }
  stage(s, no, no);
  if (wave < 4) pp_barrier();
  // (the lane number afresh, behind an asm the compiler cannot look through: computed in front of the main loop, the epilogue's row / column
  // values stay in registers the loop has none to spare for -- three of them were spilled)
  int zero = 0;
  asm volatile("" : "+v"(zero));
  const int elane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)zero));
#pragma unroll
  for (int i = 0; i < WI; ++i)
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const int col = n0 + wn * 160 + j * 32 + (elane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (elane >> 5);
        if (row < M) {
          float v = acc[i][j][e];
          float *p = C + (size_t)row * ldc + col;
          if (beta != 0.0f) v += beta * *p;
          *p = v;
        }
      }
    }
}


// ------------------------------------------------------------------------------------------------
// TN tile: C = A^T B for two CONTRACTION-MAJOR float32 operands (A: K x M, B: K x N, k the slow index) -- the weight gradients
// dW = da^T x, whose operands are the activations exactly as the recurrences leave them (K = T*B rows).  The plane path above needs
// them transposed AND split first (split_transpose_kernel: a read + write pass over both operands per GEMM); this tile takes the
// float32 rows as they are:
//   * a thread loads 16-B pieces of 4 neighbouring m of one k (8 lanes = one 128-B line of a row), splits them into hi / lo with
//     the same split_bf16 as everywhere and writes them with ds_write_b64 into a K-MAJOR LDS image: [32-m subtile][32 k][32 m]
//     bf16, rows of 64 B -- a wave's write covers 512 contiguous bytes, conflict-free;
//   * the MFMA operand (lane = m, 8 consecutive k) is the transpose of that image: two ds_read_b64_tr_b16 per fragment (each
//     16-lane group reads a 4 k x 16 m block and receives it transposed), so no shuffle and no second LDS pass;
//   * the ping-pong schedule of gemm_planes_nt256pp_af32_kernel with BOTH operands through the registers: global loads of stage
//     s + 2 between the MFMAs of the second multiply phase of stage s, their hi / lo split between the MFMAs of the first multiply
//     phase of stage s + 1 (VALU work in the shadow of the wave's own MFMAs), LDS stores in the read phase after it;
//   * split-K with an atomic (tile, split) queue on the XCDs of `xcd_mask`: partial tiles land in the workspace and
//     splitk_reduce_kernel adds them up -- the order of the splits is fixed, so the result does not depend on which workgroup
//     computed what.
// Products and k order inside a 16-k step are those of the other bf16x3 tiles (al*bh, ah*bl, ah*bh).
// ------------------------------------------------------------------------------------------------
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));

// NP = 1 (option "gemm_bf16_single"): ah*bh only -- both operands rounded to bf16 as they are staged, no lo planes in LDS.
template <int WNT, int NP = 3>
__global__ __launch_bounds__(512) void gemm_tn_f32_pp_kernel(int M, int N, int K, const float *__restrict__ A, int lda, const float *__restrict__ B,
                                                             int ldb, float *__restrict__ C, int ldc, float beta, int kchunk, int splits,
                                                             float *__restrict__ part, int tiles_m, int tiles_n, unsigned xcd_mask,
                                                             unsigned *__restrict__ queue) {
  constexpr int TBM = 256, TBN = 128 * WNT;
  constexpr int A_BYTES = TBM * 64, B_BYTES = TBN * 64;
  constexpr int STAGE = 2 * A_BYTES + 2 * B_BYTES;
  constexpr int NB = 2 * WNT;            // 16-B pieces of B per thread and stage (A: 4)
  constexpr int NMM = 4 * WNT;
  extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
  __shared__ int s_item;
  // workgroups off the XCDs of `xcd_mask` leave; the others pull (split, tile) items from ONE queue, tiles of a split next to each other
  // (an owner XCD per split -- its workgroups walking one k window together through their L2 -- measured 8-20 % slower: the L2s
  // already catch 73 % of the requests and the fixed ownership costs balance)
  {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (!((xcd_mask >> (xcc & 15u)) & 1u)) return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nt = tiles_m * tiles_n;
  const int krow = lane >> 3, c4 = 4 * (lane & 7);
  const int bsub = WNT == 2 ? wave : (wave & 3), bk0 = WNT == 2 ? 0 : 16 * (wave >> 2);
  // LDS byte offsets: this thread's pieces, and its transposing fragment reads (see tools/tr_probe: lane l of ds_read_b64_tr_b16 gets
  // column (l & 15) + 16 * ((l >> 4) & 1), rows 8 * (l >> 5) + 0..3 when lane i of a 16-lane group addresses row i / 4, columns 4 * (i % 4))
  const int st_a = wave * 2048 + krow * 64 + (lane & 7) * 8;
  const int st_b = 2 * A_BYTES + bsub * 2048 + (bk0 + krow) * 64 + (lane & 7) * 8;
  const int troff = (8 * (lane >> 5) + ((lane & 15) >> 2)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  typedef __attribute__((address_space(3))) s16x4_t *lds4_t;

  for (;;) {
    if (tid == 0) s_item = (int)atomicAdd(queue, 1u);
    __syncthreads();
    const int item = __builtin_amdgcn_readfirstlane(s_item);   // (uniform: everything derived from it -- tile origin, k window, buffer resources -- stays scalar)
    if (item >= nt * splits) return;
    const int z = item / nt, tile = item - z * nt;
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const int m0 = tm * TBM, n0 = tn * TBN;
    const int kbeg = z * kchunk, kend = min(K, kbeg + kchunk);
    const int nst = (kend - kbeg + 31) / 32;

    f32x16 acc[4][WNT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < WNT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const int acol = m0 + 32 * wave + c4, bcol = n0 + 32 * bsub + c4;
    const bool a_ok = acol < M, b_ok = bcol < N;                 // (M, N multiples of 4: a piece is inside or outside as a whole)
    // pw[q]: piece q of the stage in flight (0..3: A, 4..: B) -- first the four floats as loaded, then (convert_piece) the packed
    // words {hi01, hi23, lo01, lo23} in the same registers.  A piece beyond M / N / the k window is loaded from 16 zero bytes next to
    // the queue word instead: the select is on the ADDRESS, so nothing waits for the data inside the multiply phase the loads are
    // issued in, and the split needs no special case
    u32x4 pw[4 + NB];
    // Round 3: the eight rows of a piece through a buffer resource made on the SCALAR side per piece -- base = the piece's first row, extent =
    // its rows inside the k window -- and ONE loop-invariant lane offset (row krow, this lane's columns; 0xfffffff0 for a lane whose columns lie
    // beyond M / N): rows past the window and lanes past the edge read zeros from the range check, and the multiply phase that issues the
    // loads loses the ~18 VALU instructions per load of 64-bit address arithmetic and selects it carried (1 320 -> ~1 000 cycles,
    // tools/mb_gemm_pp.hip)
    const unsigned voff_a = a_ok ? (unsigned)((krow * lda + acol) * 4) : 0xfffffff0u;
    const unsigned voff_b = b_ok ? (unsigned)((krow * ldb + bcol) * 4) : 0xfffffff0u;
    auto load_piece = [&](int q, int k0) {                       // k0 = first k of the stage
      const int kr = q < 4 ? k0 + 8 * q : k0 + bk0 + 8 * (q - 4);                      // first of the piece's eight rows (uniform)
      const int ld = q < 4 ? lda : ldb;
      const float *base = (q < 4 ? A : B) + (size_t)min(kr, K - 1) * ld;
      int rows = min(8, kend - kr);
      asm volatile("" : "+s"(rows));                             // (kept on the scalar side: as max(0, min(8, .)) it becomes a v_med3 and the resource a waterfall loop)
      const int nrec = max(0, rows) * ld * 4;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, nrec, 0x00020000);
      pw[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, q < 4 ? voff_a : voff_b, 0, 0);
    };
    // two neighbours at a time: hi = bf16(x) of both in one v_cvt_pk_bf16_f32, lo = bf16(x - hi) likewise (the split_bf16 values)
    auto split_pair = [](float a, float b, unsigned &hw, unsigned &lw) {
      typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
      typedef float f32x2_t __attribute__((ext_vector_type(2)));
      hw = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
      const f32x2_t r = {a - __uint_as_float(hw << 16), b - __uint_as_float(hw & 0xffff0000u)};
      lw = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_t));
    };
    auto convert_piece = [&](int q) {
      unsigned h01, l01, h23, l23;
      if constexpr (NP == 3) {
        split_pair(__uint_as_float(pw[q][0]), __uint_as_float(pw[q][1]), h01, l01);
        split_pair(__uint_as_float(pw[q][2]), __uint_as_float(pw[q][3]), h23, l23);
      } else {
        typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
        typedef float f32x2_t __attribute__((ext_vector_type(2)));
        h01 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){__uint_as_float(pw[q][0]), __uint_as_float(pw[q][1])}, bf16x2_t));
        h23 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){__uint_as_float(pw[q][2]), __uint_as_float(pw[q][3])}, bf16x2_t));
        l01 = l23 = 0u;
      }
      pw[q] = (u32x4){h01, h23, l01, l23};
    };
    auto store_ab = [&](int buf) {                               // converted pieces -> the K-major image
      unsigned char *sb = qsm + buf * STAGE;
#pragma unroll
      for (int q = 0; q < 4 + NB; ++q) {
        unsigned char *p = sb + (q < 4 ? st_a + q * 512 : st_b + (q - 4) * 512);
        *reinterpret_cast<uint2 *>(p) = make_uint2(pw[q][0], pw[q][1]);
        if constexpr (NP == 3) *reinterpret_cast<uint2 *>(p + (q < 4 ? A_BYTES : B_BYTES)) = make_uint2(pw[q][2], pw[q][3]);
      }
    };
    bf16x8_t ah[4], al[4], bh[WNT], bl[WNT];
    auto tr_frag = [&](const unsigned char *p) {
      const s16x4_t x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(p));
      const s16x4_t x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(p + 256));
      return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    auto load_frags = [&](int stage, int ks) {
      const unsigned char *sb = qsm + (stage & 1) * STAGE + ks * 1024 + troff;
#pragma unroll
      for (int j = 0; j < WNT; ++j) {
        const unsigned char *p = sb + 2 * A_BYTES + (wn * WNT + j) * 2048;
        bh[j] = tr_frag(p);
        if constexpr (NP == 3) bl[j] = tr_frag(p + B_BYTES);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned char *p = sb + (wm * 4 + i) * 2048;
        ah[i] = tr_frag(p);
        if constexpr (NP == 3) al[i] = tr_frag(p + A_BYTES);
      }
    };
    // MODE 0: bare MFMAs; 1: + this thread's 4 + NB global loads of the stage that begins at k0, one after every other MFMA;
    // 2: + the split of the pieces loaded last into hi / lo words, one piece after every other MFMA
    auto multiply = [&](auto mode, int k0) {
      constexpr int MODE = decltype(mode)::value;
      constexpr int NITEM = MODE == 1 ? 4 : 4 + NB;                  // (MODE 1: the A pieces only -- B's are loaded in the read phase after)
#pragma unroll
      for (int t = 0; t < NP; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < WNT; ++j) {
            if (NP == 3 && t == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);   // small terms first
            else if (NP == 3 && t == 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            const int n = t * NMM + i * WNT + j;
            if constexpr (NP == 3) {
              if (MODE != 0 && (n & 1) && (n >> 1) < NITEM) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (MODE == 1) load_piece(n >> 1, k0);
                if constexpr (MODE == 2) convert_piece(n >> 1);
                __builtin_amdgcn_sched_barrier(0);
              }
            } else if (MODE != 0 && 2 * n < NITEM) {                   // a third of the MFMAs: two items behind every one of them
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int u = 2 * n; u < 2 * n + 2 && u < NITEM; ++u) {
                if constexpr (MODE == 1) load_piece(u, k0);
                if constexpr (MODE == 2) convert_piece(u);
              }
              __builtin_amdgcn_sched_barrier(0);
            }
          }
    };
    constexpr std::integral_constant<int, 0> bare{};
    constexpr std::integral_constant<int, 1> with_loads{};
    constexpr std::integral_constant<int, 2> with_split{};
    // prologue: stage 0 into buffer 0, stage 1 into the registers
#pragma unroll
    for (int q = 0; q < 4 + NB; ++q) load_piece(q, kbeg);
#pragma unroll
    for (int q = 0; q < 4 + NB; ++q) convert_piece(q);
    store_ab(0);
    if (nst > 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) load_piece(q, kbeg + 32);
    }
    pp_barrier();
    if (wm == 1) pp_barrier();
    // a stage = four phases: read (s, k-half 0) + loads of B(s+1) | multiply + split of the pieces of stage s + 1 (A loaded two phases ago) |
    //                        read (s, 1) + LDS stores of stage s + 1 (buffer last read two phases ago) | multiply + loads of A(s+2)
    // (round 3: all 4 + NB loads in the second multiply phase made it the longest of the four -- 1 000 cycles against a first read phase of
    // 400 whose half then waits 600 for the other half's multiply; B's NB loads moved into that read phase.  The compiler's counted vmcnt
    // waits in the split keep the order: A's pieces, the older loads, are split first)
#ifdef CTCN_GEMM_STATS
    long long gs_work[4] = {0, 0, 0, 0}, gs_wait[4] = {0, 0, 0, 0};
    const long long gs_t0 = clock64();
    long long gs_prev = gs_t0;
#endif
    auto stage = [&](int s, auto do_store, auto c1) {
      load_frags(s, 0);
      if constexpr (decltype(do_store)::value == 1) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 4; q < 4 + NB; ++q) load_piece(q, kbeg + (s + 1) * 32);       // (their registers were stored to LDS two phases ago)
      }
      PPB(0);
      if constexpr (decltype(do_store)::value == 1) multiply(with_split, 0);
      else multiply(bare, 0);
      PPB(1);
      load_frags(s, 1);
      if constexpr (decltype(do_store)::value == 1) store_ab((s + 1) & 1);
      PPB(2);
      multiply(c1, kbeg + (s + 2) * 32);
      PPB(3);
    };
    int s = 0;
    for (; s + 2 < nst; ++s) stage(s, with_loads, with_loads);
#ifdef CTCN_GEMM_STATS
    if (lane == 0 && (wave & 3) == 0 && item == 0 && g_gemm_stats) {
      long long *o = g_gemm_stats + (wave >> 2) * 16;
      for (int i = 0; i < 4; ++i) { o[i] = gs_work[i]; o[4 + i] = gs_wait[i]; }
      o[8] = clock64() - gs_t0; o[9] = nst - 2; o[10] = 0;
    }
#endif
    if (s + 1 < nst) { stage(s, with_loads, bare); ++s; }
    stage(s, bare, bare);
    if (wm == 0) pp_barrier();

    float *o = splits > 1 ? part + (size_t)z * M * N : C;
    const int ldo = splits > 1 ? N : ldc;
    const float bt = splits > 1 ? 0.0f : beta;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < WNT; ++j) {
        const int col = n0 + wn * 32 * WNT + j * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * 128 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
          if (row < M && col < N) {
            float v = acc[i][j][e];
            float *p = o + (size_t)row * ldo + col;
            if (bt != 0.0f) v += bt * *p;
            *p = v;
          }
        }
      }
    __syncthreads();
  }
}

__global__ void splitk_reduce_kernel(const float *__restrict__ ws, float *__restrict__ C, int M, int N, int ldc,
                                     int splits, float beta) {
  const size_t total = (size_t)M * N;
  // the partials are summed in split order (the result does not depend on the launch), eight loads in flight at a time.
  // Round 5: 16-B loads / stores and a 32-bit division per FOUR outputs where the shape allows (every product of the training step:
  // N, ldc multiples of 4, 16-B aligned C and partials) -- the same additions in the same order, bit-identical to the scalar form below.
  if ((N & 3) == 0 && (ldc & 3) == 0 && (((uintptr_t)C | (uintptr_t)ws) & 15) == 0 && total < ((size_t)1 << 33)) {
    const unsigned n4 = (unsigned)(N >> 2), total4 = (unsigned)(total >> 2);
    const float4 *w4 = reinterpret_cast<const float4 *>(ws);
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
      float4 s = {0.0f, 0.0f, 0.0f, 0.0f};
      int z = 0;
      for (; z + 8 <= splits; z += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = w4[(size_t)(z + u) * total4 + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
      }
      for (; z < splits; ++z) { const float4 v = w4[(size_t)z * total4 + i]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
      const unsigned m = i / n4, n = (i - m * n4) << 2;
      float4 *p = reinterpret_cast<float4 *>(C + (size_t)m * ldc + n);
      if (beta != 0.0f) { const float4 o = *p; s.x += beta * o.x; s.y += beta * o.y; s.z += beta * o.z; s.w += beta * o.w; }
      *p = s;
    }
    return;
  }
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    float s = 0.0f;
    int z = 0;
    for (; z + 8 <= splits; z += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ws[(size_t)(z + u) * total + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; z < splits; ++z) s += ws[(size_t)z * total + i];
    const size_t m = i / N, n = i - m * N;
    float *p = C + m * ldc + n;
    if (beta != 0.0f) s += beta * *p;
    *p = s;
  }
}

__global__ void transpose01_kernel(const float *__restrict__ in, float *__restrict__ out, int A, int B, int C) {
  // out[b][a][c] = in[a][b][c]
  const size_t total = (size_t)A * B * C;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = i % C;
    const size_t ab = i / C;
    const int a = ab % A;     // out index = (b*A + a)*C + c
    const int b = ab / A;
    out[i] = in[((size_t)a * B + b) * C + c];
  }
}

}  // namespace

// ================================================================================================
// Host side.  plan_gemm decides -- which of the nine kernel families, its tiling, the split-K count, the operand split passes, the
// workspace layout, the grid -- by arithmetic alone; gemm_core carries a plan out.  ctcn_diag_gemm_plan shows the plan to the CPU tests.
// ================================================================================================
enum GemmPath { GP_F32 = 0, GP_F32_QUEUE, GP_BF16X3, GP_PLANES128, GP_PLANES128_QUEUE, GP_PLANES256, GP_PLANES256_AF32, GP_PLANES256_QUEUE, GP_TN };
enum SplitPass { SP_NONE = 0, SP_ROWS, SP_TRANSPOSE, SP_TRANSPOSE_QUEUE };      // how an operand becomes bf16 planes in the workspace
struct GemmShape { int transA, transB, M, N, K, lda, ldb, ldc, precision, b_shift; };
struct GemmOptions { int tile256, a_inline, tn, big_tiles, tn_splits_xcd, tn_splits_force; };
struct GemmEnv {
  int a_mod16, b_mod16;          // A and B modulo 16 bytes
  bool has_ws;
  size_t ws_bytes;
  unsigned xcd_allow;            // 0 = whole device; otherwise the XCDs the workgroups may run on (side stream next to a recurrence)
  bool same_a, same_b;           // the workspace still holds this call's A / B planes (GemmPlanes)
  int cus, xcds;
  GemmOptions opt;
};
struct GemmPlan {
  GemmPath path;
  int ti, tj;                    // workgroup tile = 64 ti x 64 tj
  int wnt;                       // 256-row tiles: 32-column MFMA tiles per wave
  int splits, kchunk;            // split-K
  SplitPass split_a, split_b;
  int Kp;                        // plane paths: K rounded up to the planes' 64-k slabs
  size_t off_al, off_bh, off_bl, off_part, off_queue;      // workspace layout (bytes): [Ah | Al | Bh | Bl | split-K partials ... queue words]
  int tiles_m, tiles_n;
  unsigned grid_x, grid_y;
  bool vecA, vecB;               // direct kernels: 16-B loads of the operand
  unsigned xcd_mask;             // TN tile: the XCDs its queue runs on
};
static bool uses_planes(GemmPath p) { return p >= GP_PLANES128 && p <= GP_PLANES256_QUEUE; }
static GemmOptions gemm_options() {
  return {ctcn_get_option("gemm_tile256"), ctcn_get_option("gemm_a_inline"), ctcn_get_option("gemm_tn"), ctcn_opt_gemm_big_tiles(),
          ctcn_get_option("tn_splits_xcd"), ctcn_get_option("tn_splits_force")};
}
static int check_gemm_shape(const GemmShape &g) {
  CTCN_REQUIRE(g.precision == 0 || g.precision == 1, "ctcn_gemm: precision %d (0 = f32 MFMA, 1 = bf16x3 split MFMA)", g.precision);
  CTCN_REQUIRE(g.M > 0 && g.N > 0 && g.K >= 0, "ctcn_gemm: bad dims M=%d N=%d K=%d", g.M, g.N, g.K);
  CTCN_REQUIRE(g.lda >= (g.transA ? g.M : g.K) && g.ldb >= (g.transB ? g.K : g.N) && g.ldc >= g.N, "ctcn_gemm: leading dim too small");
  return CTCN_OK;
}
// pre-split planes in the workspace: Ah | Al (M x Kp each) | Bh | Bl (N x Kp each), then the split-K partials
struct PlaneLayout { int Kp; size_t a_el, b_el, bytes; };
static PlaneLayout plane_layout(int M, int N, int K) {
  const int Kp = ceil_div(K, PBK) * PBK;
  const size_t a_el = (size_t)M * Kp, b_el = (size_t)N * Kp;
  return {Kp, a_el, b_el, align_up(2 * (a_el + b_el) * sizeof(unsigned short), 256)};
}
// the TN tile (gemm_tn_f32_pp_kernel) takes C = A^T B with 16-B aligned rows of whole float4 pieces, large K, and a workspace for its
// queue word (+ the split-K partials)
static bool tn_eligible(const GemmShape &g, const GemmEnv &e) {
  return g.precision == 1 && g.transA && !g.transB && e.has_ws && e.ws_bytes >= 1024 && e.opt.tn != 0 && g.M >= 128 && g.N >= 32 && g.K >= 1024 &&
         g.M % 4 == 0 && g.N % 4 == 0 && g.lda % 4 == 0 && g.ldb % 4 == 0 && e.a_mod16 == 0 && e.b_mod16 == 0 &&
         g.lda < (1 << 24) && g.ldb < (1 << 24);                 // (eight rows of a piece behind one 32-bit buffer offset)
}

static GemmPlan plan_gemm(const GemmShape &g, const GemmEnv &e) {
  const int M = g.M, N = g.N, K = g.K;
  const size_t mn_bytes = (size_t)M * N * sizeof(float);
  GemmPlan p = {};
  p.splits = 1;
  // the last 256 bytes of the workspace hold the work queue of the XCD-filtered variants and of the TN tile
  p.off_queue = e.ws_bytes >= 256 ? (e.ws_bytes - 256) & ~(size_t)255 : 0;
  if (tn_eligible(g, e) && g.b_shift == 0) {
    // both operands contraction-major (weight gradients): the TN tile reads the float32 rows as they are -- no plane pass
    p.path = GP_TN;
    p.wnt = ceil_div(N, 256) * 256 == ceil_div(N, 128) * 128 ? 2 : 1;     // (N = 640 as 3 x 256 or 5 x 128: the same time)
    p.ti = 4; p.tj = 2 * p.wnt;
    p.tiles_m = ceil_div(M, 256); p.tiles_n = ceil_div(N, 128 * p.wnt);
    // the CUs the launch may run on -- 256, or (round 5, option "tn_splits_xcd") the CUs of the XCDs of xcd_allow: one round of items there
    // instead of two rounds of half-length items (each item pays a prologue, a 128-KB partial store and its share of the reduce pass)
    int cus = 256;
    if (e.xcd_allow && e.opt.tn_splits_xcd != 0) {
      const int nx = std::max(1, std::min(e.xcds, 16));
      cus = std::max(e.cus / nx * __builtin_popcount(e.xcd_allow & ((1u << nx) - 1u)), 32);
    }
    const int tiles = p.tiles_m * p.tiles_n;
    int s = std::min(std::max(cus / tiles, 1), std::max(K / 512, 1));      // <= 256 items: one round on a whole device
    s = std::min(s, 32);                                                    // (a handful of tiles: the reduce pass over the partials would take over)
    if (const int f = e.opt.tn_splits_force) s = std::min(f, std::max(K / 64, 1));       // (development)
    s = std::min(s, (int)((e.ws_bytes - 512) / mn_bytes));                  // the partials: splits * M * N floats at the workspace's start
    if (s < 2) s = 1;
    p.kchunk = ceil_div(ceil_div(K, s), 32) * 32;
    p.splits = ceil_div(K, p.kchunk);
    const int nx = std::min(e.xcds, 16);
    p.xcd_mask = e.xcd_allow ? e.xcd_allow : (nx > 1 ? (1u << nx) - 1u : 0xffffu);
    p.grid_x = e.cus; p.grid_y = 1;
    return p;
  }
  const PlaneLayout lay = plane_layout(M, N, K);
  if (g.precision == 1 && K >= 64 && e.has_ws && e.ws_bytes >= lay.bytes + 1024) {
    const int Kp = p.Kp = lay.Kp;
    p.off_al = lay.a_el * sizeof(unsigned short); p.off_bh = 2 * p.off_al; p.off_bl = p.off_bh + lay.b_el * sizeof(unsigned short);
    p.off_part = lay.bytes;
    const size_t part_bytes = e.ws_bytes - lay.bytes - 512;
    p.kchunk = Kp;
    const SplitPass pass_a = g.transA == 0 ? SP_ROWS : (e.xcd_allow ? SP_TRANSPOSE_QUEUE : SP_TRANSPOSE);
    const SplitPass pass_b = g.transB != 0 ? SP_ROWS : (e.xcd_allow ? SP_TRANSPOSE_QUEUE : SP_TRANSPOSE);
    p.split_b = e.same_b ? SP_NONE : pass_b;
    // activation-sized products (M = T*B): the 256-row tiles, when they give the device at least ~0.75 workgroups per CU; a
    // row-major A (k contiguous) is then split while it is staged, without a plane pass of its own
    const int wnt256 = (N % 256 == 0 || (N > 512 && ceil_div(N, 256) * 256 - N <= N / 8)) ? 2 : 1;
    const int t256_m = ceil_div(M, 256), t256_n = ceil_div(N, 128 * wnt256);
    const bool use256 = !e.xcd_allow && e.opt.tile256 != 0 && M >= 1024 && N >= 96 && (long)t256_m * t256_n * 4 >= (long)e.cus * 3;
    // (every N-tile converts its A rows again.  Stand-alone the inline split now wins at every shape of the bench configurations --
    // 25 600 x 1 280 x 640: 134 vs 150 us, 25 600 x 640 x 2 560: 278 vs 354 us, 25 600 x 2 560 x 640 (10 N-tiles): 253 vs 262 us,
    // 76 800 x 3 072 x 1 024 (12 N-tiles): 1 333 vs 1 351 us -- but with a limit of 16 N-tiles instead of 5 no step got faster (cfg2
    // 13.74 / 13.75 ms in an A/B inside one session, cfg4 58.2 vs 57.6-58.3), so the limit stays where it was tested longest)
    const bool a_inline = use256 && !e.same_a && !g.transA && e.opt.a_inline != 0 && K >= 32 && K % 4 == 0 && g.lda % 4 == 0 && e.a_mod16 == 0 &&
                          t256_n <= 5;
    p.split_a = (a_inline || e.same_a) ? SP_NONE : pass_a;
    // side stream: the 256-row tiles from a queue when they fill the allowed XCDs' CUs at least 3/4 in whole rounds of one tile per CU
    // (the chunk GEMMs of the pipelined input projection are sized for that: rnn.hip)
    bool queue256 = false;
    if (e.xcd_allow && e.opt.tile256 != 0 && M >= 1024 && N >= 96) {
      const int cus = e.cus / std::max(1, std::min(e.xcds, 16)) * __builtin_popcount(e.xcd_allow);
      const int t256 = t256_m * t256_n, rounds = ceil_div(t256, std::max(cus, 1));
      queue256 = cus > 0 && t256 * 4 >= rounds * cus * 3;
    }
    if (use256 || queue256) {
      p.path = a_inline ? GP_PLANES256_AF32 : (use256 ? GP_PLANES256 : GP_PLANES256_QUEUE);
      p.wnt = wnt256; p.ti = 4; p.tj = 2 * wnt256;
      p.tiles_m = t256_m; p.tiles_n = t256_n;
      p.grid_x = queue256 ? e.cus : t256_m * t256_n; p.grid_y = 1;
      return p;
    }
    // tile shape: 128x128 (two workgroups per CU).  Option gemm_big_tiles: 256x128 / 128x256 tiles (one per CU, 96 KB of LDS)
    // when they fill the device at least once without more padding -- 25 % fewer LDS fragment reads per MFMA, yet measured
    // 7 % SLOWER at cfg2 / 4 % at cfg4 (the second resident workgroup hides the staging barriers better), so off by default
    p.ti = p.tj = 2; p.tiles_m = ceil_div(M, BM); p.tiles_n = ceil_div(N, BN);
    {
      const long t22 = (long)p.tiles_m * p.tiles_n * 128 * 128;
      const int m42 = ceil_div(M, 256), n42 = ceil_div(N, 128), m24 = ceil_div(M, 128), n24 = ceil_div(N, 256);
      const long t42 = (long)m42 * n42 * 256 * 128, t24 = (long)m24 * n24 * 128 * 256;
      const bool ok42 = m42 * n42 >= e.cus && t42 <= t22 + t22 / 32, ok24 = m24 * n24 >= e.cus && t24 <= t22 + t22 / 32;
      if (e.opt.big_tiles && (ok42 || ok24)) {
        if (ok24 && (!ok42 || t24 <= t42)) { p.tj = 4; p.tiles_m = m24; p.tiles_n = n24; }
        else { p.ti = 4; p.tiles_m = m42; p.tiles_n = n42; }
      }
    }
    const int pnt = p.tiles_m * p.tiles_n;
    if (pnt < 256 && Kp >= 1024 && part_bytes >= 2 * mn_bytes) {
      p.splits = std::min(std::min(ceil_div(512, pnt), Kp / 512), (int)(part_bytes / mn_bytes));
      if (p.splits < 2) p.splits = 1;
    }
    if (p.splits > 1) {
      p.kchunk = ceil_div(ceil_div(Kp, p.splits), PBK) * PBK;
      p.splits = ceil_div(Kp, p.kchunk);
    }
    p.path = e.xcd_allow ? GP_PLANES128_QUEUE : GP_PLANES128;
    p.grid_x = e.xcd_allow ? 2 * e.cus : pnt; p.grid_y = e.xcd_allow ? 1 : p.splits;
    return p;
  }
  // the direct kernels: 128 x 128 tiles, operands staged (and, precision 1, split) from the float32 matrices
  p.ti = p.tj = 2; p.tiles_m = ceil_div(M, BM); p.tiles_n = ceil_div(N, BN);
  const int nt = p.tiles_m * p.tiles_n;
  if (nt < 256 && K >= 512 && e.has_ws && e.ws_bytes >= 2 * mn_bytes) {
    p.splits = std::min(std::min(ceil_div(512, nt), K / 256), (int)(e.ws_bytes / mn_bytes));
    if (p.splits < 2) p.splits = 1;
  }
  p.kchunk = K;
  if (p.splits > 1) {
    p.kchunk = ceil_div(ceil_div(K, p.splits), XBK) * XBK;
    p.splits = ceil_div(K, p.kchunk);
  }
  p.vecA = e.a_mod16 == 0 && g.lda % 4 == 0;
  p.vecB = e.b_mod16 == 0 && g.ldb % 4 == 0;
  // precision 0 on a side stream next to a persistent recurrence: tiles from an atomic queue, workgroups off the allowed XCDs exit
  const bool queued = g.precision == 0 && e.xcd_allow && e.has_ws && e.ws_bytes >= (p.splits > 1 ? p.splits * mn_bytes : 0) + 512;
  p.path = g.precision == 1 ? GP_BF16X3 : (queued ? GP_F32_QUEUE : GP_F32);
  p.grid_x = queued ? 2 * e.cus : nt; p.grid_y = queued ? 1 : p.splits;
  return p;
}

extern "C" int ctcn_diag_gemm_plan(int transA, int transB, int M, int N, int K, int lda, int ldb, int ldc, int precision, int b_shift, int a_mod16,
                                   int b_mod16, int has_ws, size_t ws_bytes, unsigned xcd_allow, int same_a, int same_b, int cus, int xcds, int *out) {
  const GemmShape g = {transA, transB, M, N, K, lda, ldb, ldc, precision, b_shift};
  if (const int rc = check_gemm_shape(g)) return rc;
  CTCN_REQUIRE(out && cus > 0 && xcds > 0 && a_mod16 >= 0 && a_mod16 < 16 && b_mod16 >= 0 && b_mod16 < 16, "ctcn_diag_gemm_plan: bad args");
  const GemmPlan p = plan_gemm(g, {a_mod16, b_mod16, has_ws != 0, ws_bytes, xcd_allow, same_a != 0, same_b != 0, cus, xcds, gemm_options()});
  const int v[CTCN_GEMM_PLAN_INTS] = {p.path, p.ti, p.tj, p.wnt, p.splits, p.kchunk, p.split_a, p.split_b, (int)p.grid_x, (int)p.grid_y, p.vecA, p.vecB};
  memcpy(out, v, sizeof(v));
  return CTCN_OK;
}

// option "gemm_bf16_single" (default 0): 1 = the 256-row tiles (plane, float32-A and TN forms: every product of T*B rows) multiply the bf16 roundings of
// their operands ONCE (ah*bh, f32 accumulate) instead of the three bf16x3 products -- the "bf16 tolerance" BASELINE.json's north_star states
// (loss / activations within 1e-3), against the default's f32-equivalent 1e-5.  The recurrent matmul and the small tiles keep bf16x3.
static bool bf16_single() { return ctcn_get_option("gemm_bf16_single") != 0; }

// f(integral_constant) for a runtime value that takes one of two / three forms
template <class F> static int with_wnt(int wnt, F f) { return wnt == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 1>{}); }
template <class F> static void with_trans(int ta, int tb, F f) {
  if (ta) { if (tb) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else    { if (tb) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}
// one of the 256-row kernels: 512 threads, two stages of (256 + 128 wnt) rows x 64 B x 2 planes of dynamic LDS
template <class Kern, class... Args>
static int launch_tile256(Kern kern, unsigned grid, int wnt, hipStream_t st, Args... args) {
  const size_t lds = (size_t)2 * (2 * 256 * 64 + 2 * 128 * wnt * 64);
  CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, args...);
  return CTCN_OK;
}
// one operand -> its hi / lo bf16 planes (rows x Kp, k contiguous); `queue`: the next free queue word of an XCD-filtered pass
static void launch_split(SplitPass pass, hipStream_t st, const float *src, int ld, int rows, int K, int Kp, unsigned short *hi, unsigned short *lo, int shift,
                         unsigned xcd_allow, unsigned *queue) {
  if (pass == SP_ROWS) {                      // src[row*ld + k]
    const size_t total = (size_t)rows * (Kp / 4);
    hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)std::min((size_t)8192, ceil_div_z(total, 256))), dim3(256), 0, st, src, ld, rows, K, Kp, hi, lo);
  } else if (pass == SP_TRANSPOSE_QUEUE) {    // src[k*ld + row] -> transpose
    hipLaunchKernelGGL(split_transpose_queue_kernel, dim3(ctcn_opt_side_split_wgs() * ctcn_device_cus()), dim3(256), 0, st, src, ld, K, rows, Kp, hi, lo,
                       ceil_div(rows, 64), ceil_div(Kp, 64), xcd_allow, queue, shift);
  } else if (pass == SP_TRANSPOSE) {
    hipLaunchKernelGGL(split_transpose_kernel, dim3(ceil_div(rows, 64), ceil_div(Kp, 64)), dim3(256), 0, st, src, ld, K, rows, Kp, hi, lo, shift);
  }
}

// xcd_allow: 0 = whole device; otherwise the XCDs the GEMM workgroups may run on
// b_shift: ctcn_gemm_shift_b's shift of B along k, applied while B is split (plane path only)
static int gemm_core(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C,
                     int ldc, float beta, int precision, void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow, GemmPlanes *planes, int b_shift) {
  GemmPlanes scratch_planes;                  // a caller without a sequence: nothing to reuse, nothing remembered
  GemmPlanes &pl = planes ? *planes : scratch_planes;
  const bool want_same_a = pl.same_a, want_same_b = pl.same_b;
  pl.same_a = pl.same_b = false;              // one-shot
  const GemmShape g = {transA, transB, M, N, K, lda, ldb, ldc, precision, b_shift};
  if (const int rc = check_gemm_shape(g)) return rc;
  CTCN_REQUIRE(A && B && C, "ctcn_gemm: null pointer");
  // A, B and C may start on any 4 bytes (every 16-byte access to them is chosen from the pointer: vecA / vecB, split_transpose_tile, the inline
  // A split, the TN tile, the split-K reduce); the workspace may not: bf16 planes, partials and queue words are carved from it by offset alone
  CTCN_REQUIRE(!ws || (uintptr_t)ws % 16 == 0, "ctcn_gemm: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char *const wsb = (char *)ws;
  const void *bh_here = wsb + 2 * plane_layout(M, N, K).a_el * sizeof(unsigned short);       // where this call's B planes would lie
  GemmEnv e = {(int)((uintptr_t)A & 15), (int)((uintptr_t)B & 15), ws != nullptr, ws_bytes, xcd_allow, false, false, ctcn_device_cus(), 0, gemm_options()};
  e.same_a = want_same_a && pl.a_valid && pl.A == A && pl.lda == lda && pl.M == M && pl.Ka == K && pl.transA == transA && pl.ws_a == ws && pl.st_a == (void *)st;
  e.same_b = want_same_b && pl.b_valid && pl.B == B && pl.ldb == ldb && pl.N == N && pl.Kb == K && pl.transB == transB && pl.shift == b_shift &&
             pl.ws_b == ws && pl.st_b == (void *)st && pl.bh == bh_here;
  // (the XCD count is read by the side-stream rules and the TN tile only, and its first query probes the device: calls that cannot need it do not ask)
  if (xcd_allow || tn_eligible(g, e)) e.xcds = ctcn_device_xcds();
  const GemmPlan p = plan_gemm(g, e);

  unsigned short *ah = (unsigned short *)wsb, *al = (unsigned short *)(wsb + p.off_al), *bh = (unsigned short *)(wsb + p.off_bh),
                 *bl = (unsigned short *)(wsb + p.off_bl);
  float *part = p.splits > 1 ? (float *)(wsb + p.off_part) : nullptr;
  unsigned *queue = (unsigned *)(wsb + p.off_queue);
  pl.a_valid = pl.b_valid = false;            // what the workspace holds after this call
  if (uses_planes(p.path)) {
    pl.B = B; pl.ldb = ldb; pl.N = N; pl.Kb = K; pl.transB = transB; pl.shift = b_shift; pl.ws_b = ws;
    pl.st_b = (void *)st; pl.bh = (const void *)bh; pl.b_valid = true;
    if (p.path != GP_PLANES256_AF32) {
      pl.A = A; pl.lda = lda; pl.M = M; pl.Ka = K; pl.transA = transA; pl.ws_a = ws; pl.st_a = (void *)st;
      pl.a_valid = true;
    }
    if (xcd_allow) CTCN_HIP(hipMemsetAsync(queue, 0, 16, st));
    int nq = 0;      // queue words 1, 2: the operand splits
    launch_split(p.split_a, st, A, lda, M, K, p.Kp, ah, al, 0, xcd_allow, queue + (p.split_a == SP_TRANSPOSE_QUEUE ? ++nq : 0));
    launch_split(p.split_b, st, B, ldb, N, K, p.Kp, bh, bl, b_shift, xcd_allow, queue + (p.split_b == SP_TRANSPOSE_QUEUE ? ++nq : 0));
    CTCN_LAUNCH_CHECK();
  }
  const int tiles_m = p.tiles_m, tiles_n = p.tiles_n, Kp = p.Kp, kchunk = p.kchunk, splits = p.splits;
  const dim3 grid(p.grid_x, p.grid_y);
  int rc = CTCN_OK;
  switch (p.path) {
    case GP_TN:
      CTCN_HIP(hipMemsetAsync(queue, 0, 128, st));              // the queue word, and at +64 the 16 zero bytes pieces outside the operands are loaded from
      rc = with_wnt(p.wnt, [&](auto W) {
        constexpr int WNT = decltype(W)::value;
        return launch_tile256(bf16_single() ? gemm_tn_f32_pp_kernel<WNT, 1> : gemm_tn_f32_pp_kernel<WNT, 3>, p.grid_x, WNT, st, M, N, K, A, lda, B, ldb, C, ldc,
                              beta, kchunk, splits, part, tiles_m, tiles_n, p.xcd_mask, queue);
      });
      break;
    case GP_PLANES256_AF32:
      rc = with_wnt(p.wnt, [&](auto W) {
        constexpr int WNT = decltype(W)::value;
        return launch_tile256(bf16_single() ? gemm_planes_nt256pp_af32_kernel<WNT, 1> : gemm_planes_nt256pp_af32_kernel<WNT, 3>, p.grid_x, WNT, st, M, N, K, Kp,
                              A, lda, (const unsigned short *)bh, (const unsigned short *)bl, C, ldc, beta, tiles_m, tiles_n);
      });
      break;
    case GP_PLANES256:
      rc = with_wnt(p.wnt, [&](auto W) {
        constexpr int WNT = decltype(W)::value;
        return launch_tile256(bf16_single() ? gemm_planes_nt256pp_kernel<WNT, 1> : gemm_planes_nt256pp_kernel<WNT, 3>, p.grid_x, WNT, st, M, N, Kp,
                              (const unsigned short *)ah, (const unsigned short *)al, (const unsigned short *)bh, (const unsigned short *)bl, C, ldc, beta,
                              tiles_m, tiles_n, ctcn_get_option("gemm_dbg"));
      });
      break;
    case GP_PLANES256_QUEUE:
      rc = with_wnt(p.wnt, [&](auto W) {
        constexpr int WNT = decltype(W)::value;
        return launch_tile256(bf16_single() ? gemm_planes_nt256pp_queue_kernel<WNT, 1> : gemm_planes_nt256pp_queue_kernel<WNT, 3>, p.grid_x, WNT, st, M, N, Kp,
                              (const unsigned short *)ah, (const unsigned short *)al, (const unsigned short *)bh, (const unsigned short *)bl, C, ldc, beta,
                              tiles_m, tiles_n, xcd_allow, queue);
      });
      break;
    case GP_PLANES128:
    case GP_PLANES128_QUEUE: {
      // one of the three tile shapes (dynamic LDS = 2 planes x (BM + BN) rows x 128 B)
      auto launch = [&](auto TI_, auto TJ_) {
        constexpr int TI = decltype(TI_)::value, TJ = decltype(TJ_)::value;
        const size_t lds = (size_t)2 * (64 * TI + 64 * TJ) * 128;
        if (p.path == GP_PLANES128_QUEUE) {
          auto kern = gemm_planes_nt_queue_kernel<TI, TJ>;
          if (lds > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, M, N, Kp, ah, al, bh, bl, C, ldc, beta, kchunk, part, tiles_m, tiles_n, splits, xcd_allow, queue);
        } else {
          auto kern = gemm_planes_nt_kernel<TI, TJ>;
          if (lds > 64 * 1024) CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, M, N, Kp, ah, al, bh, bl, C, ldc, beta, kchunk, part, tiles_m, tiles_n);
        }
        return (int)CTCN_OK;
      };
      constexpr std::integral_constant<int, 2> two{};
      constexpr std::integral_constant<int, 4> four{};
      rc = p.ti == 4 ? launch(four, two) : (p.tj == 4 ? launch(two, four) : launch(two, two));
      break;
    }
    case GP_F32_QUEUE:
      CTCN_HIP(hipMemsetAsync(queue, 0, 4, st));
      with_trans(transA, transB, [&](auto TA, auto TB) {
        hipLaunchKernelGGL((gemm_f32_queue_kernel<decltype(TA)::value, decltype(TB)::value>), grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, beta, kchunk,
                           part, tiles_m, tiles_n, p.vecA, p.vecB, splits, xcd_allow, queue);
      });
      break;
    case GP_F32:
      with_trans(transA, transB, [&](auto TA, auto TB) {
        hipLaunchKernelGGL((gemm_f32_kernel<decltype(TA)::value, decltype(TB)::value>), grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, beta, kchunk, part,
                           tiles_m, tiles_n, p.vecA, p.vecB);
      });
      break;
    case GP_BF16X3:
      with_trans(transA, transB, [&](auto TA, auto TB) {
        hipLaunchKernelGGL((gemm_bf16x3_kernel<decltype(TA)::value, decltype(TB)::value>), grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, beta, kchunk,
                           part, tiles_m, tiles_n, p.vecA, p.vecB);
      });
      break;
  }
  if (rc) return rc;
  CTCN_LAUNCH_CHECK();
  if (splits > 1) {                           // the partials are summed in split order, whichever workgroup made them
    const size_t total = (size_t)M * N;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((int)std::min((size_t)2048, ceil_div_z(total, 256))), dim3(256), 0, st, (const float *)part, C, M, N, ldc,
                       splits, beta);
    CTCN_LAUNCH_CHECK();
  }
  return CTCN_OK;
}

int ctcn_gemm_on_xcds(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C,
                      int ldc, float beta, int precision, void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow, GemmPlanes *planes) {
  return gemm_core(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, beta, precision, ws, ws_bytes, stream, xcd_allow, planes, 0);
}
extern "C" int ctcn_diag_gemm_on_xcds(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                                      float beta, int precision, void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow) {
  return gemm_core(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, beta, precision, ws, ws_bytes, stream, xcd_allow, nullptr, 0);
}

// C = A^T * shift_k(B) for contraction-major A (K x M) and B (K x N): B_eff[k] = B[k - shift] when 0 <= k - shift < K, else 0 --
// the recurrent weight gradient dW_hh = da^T h_prev with h_prev = y delayed (forward direction) or advanced (reverse) by one
// timestep.  On the bf16x3 plane path the shift is applied while B is split, so that A = da^T keeps the SAME K window as in
// dW_ih = da^T x and its planes can be reused (GemmPlanes::same_a); elsewhere the window is narrowed instead.
int ctcn_gemm_shift_b(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, float beta, int precision,
                      void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow, int shift, GemmPlanes *planes) {
  const int as = shift < 0 ? -shift : shift;
  CTCN_REQUIRE(as < K, "ctcn_gemm_shift_b: |shift| %d >= K %d", as, K);
  // the plane path with the whole window, unless the narrowed window would go to the TN tile, which has no planes to share (both answers
  // are the same on any device: the XCD count only sizes things inside a path)
  const GemmEnv e = {(int)((uintptr_t)A & 15), (int)((uintptr_t)B & 15), ws != nullptr, ws_bytes, xcd_allow, false, false, ctcn_device_cus(), 0, gemm_options()};
  const bool plane = uses_planes(plan_gemm({1, 0, M, N, K, lda, ldb, ldc, precision, shift}, e).path) &&
                     plan_gemm({1, 0, M, N, K - as, lda, ldb, ldc, precision, 0}, e).path != GP_TN;
  if (!plane) {
    if (planes) planes->same_a = false;
    const float *A2 = shift > 0 ? A + (size_t)as * lda : A, *B2 = shift < 0 ? B + (size_t)as * ldb : B;
    return gemm_core(1, 0, M, N, K - as, A2, lda, B2, ldb, C, ldc, beta, precision, ws, ws_bytes, stream, xcd_allow, planes, 0);
  }
  return gemm_core(1, 0, M, N, K, A, lda, B, ldb, C, ldc, beta, precision, ws, ws_bytes, stream, xcd_allow, planes, shift);
}

// The dW_ih / dW_hh pair of ctcn_rnn_bwd_weights as one call, for tests: C1 = A^T B1 through ctcn_gemm_on_xcds, then C2 = A2^T shift_k(B2)
// through ctcn_gemm_shift_b, both with one GemmPlanes; reuse != 0 sets same_a in between as the layer does (A2 == A there; an A2 that differs
// must be refused by the guard and split again).  reuse == 2 also fills A's K x M window with 0xFF bytes (NaN) between the two products: a
// second product that reads A instead of the planes the first one left shows it in every output.
extern "C" int ctcn_diag_gemm_shift_b_pair(int M, int N1, int N2, int K, const float *A, int lda, const float *B1, int ldb1, float *C1, int ldc1,
                                           const float *A2, const float *B2, int ldb2, float *C2, int ldc2, float beta, int precision, void *ws,
                                           size_t ws_bytes, void *stream, unsigned xcd_allow, int shift, int reuse) {
  GemmPlanes pl;
  if (const int rc = ctcn_gemm_on_xcds(1, 0, M, N1, K, A, lda, B1, ldb1, C1, ldc1, beta, precision, ws, ws_bytes, stream, xcd_allow, &pl)) return rc;
  if (reuse) pl.same_a = true;
  if (reuse == 2) CTCN_HIP(hipMemset2DAsync(const_cast<float *>(A), (size_t)lda * sizeof(float), 0xFF, (size_t)M * sizeof(float), (size_t)K, (hipStream_t)stream));
  return ctcn_gemm_shift_b(M, N2, K, A2, lda, B2, ldb2, C2, ldc2, beta, precision, ws, ws_bytes, stream, xcd_allow, shift, &pl);
}

extern "C" int ctcn_gemm(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B,
                         int ldb, float *C, int ldc, float beta, int precision, void *ws, size_t ws_bytes,
                         void *stream) {
  return gemm_core(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, beta, precision, ws, ws_bytes, stream, 0u, nullptr, 0);
}

// ---- the dx product: C = A B, A row-major float32 (M x K), B row-major K x N -------------------------------------------------------------
// ctcn_gemm(0, 0, ...) with one more tile to choose from: gemm_af32_n320pp_kernel (256 x 320) where N is a multiple of 320 and the tile count
// says it wins.  A planner of its own: plan_gemm's answers stay what they are for every caller.  Same bits either way.
// DX_WIDE_COST: time of one round of 256 x 320 tiles over one round of 256 x 128 float32-A tiles at N = 640, K = 2 560 on an MI355X: 216 us
// (200 tiles, M = 25 600) against 115.5 us (250 tiles, M = 12 800) -- tools/mb_gemm_pp.hip modes 4 and 1, profiles/dx_tile_ab.txt.
constexpr double DX_WIDE_COST = 1.87;
struct DxPlan { bool eligible, wide; int tiles_wide, tiles_128; };
static DxPlan plan_dx(int M, int N, int K, int lda, int precision, int a_mod16, bool has_ws, size_t ws_bytes, int cus, int opt_wide, bool single) {
  DxPlan p = {};
  p.tiles_128 = ceil_div(M, 256) * ceil_div(N, 128);
  p.eligible = precision == 1 && !single && N % 320 == 0 && K >= 64 && K % 4 == 0 && lda % 4 == 0 && a_mod16 == 0 && has_ws &&
               ws_bytes >= plane_layout(0, N, K).bytes;
  if (!p.eligible) return p;
  p.tiles_wide = ceil_div(M, 256) * (N / 320);
  // by rounds of one tile per CU: the wide tile where its rounds, each DX_WIDE_COST times as long, take less time than the 256 x 128 tile's
  const int c = std::max(cus, 1);
  p.wide = opt_wide == 2 || (opt_wide == 1 && ceil_div(p.tiles_wide, c) * DX_WIDE_COST < (double)ceil_div(p.tiles_128, c));
  return p;
}
extern "C" int ctcn_diag_dx_plan(int M, int N, int K, int lda, int precision, int a_mod16, int has_ws, size_t ws_bytes, int cus, int *out) {
  CTCN_REQUIRE(out && M > 0 && N > 0 && K >= 0 && cus > 0 && a_mod16 >= 0 && a_mod16 < 16, "ctcn_diag_dx_plan: bad args");
  const DxPlan p = plan_dx(M, N, K, lda, precision, a_mod16, has_ws != 0, ws_bytes, cus, ctcn_get_option("gemm_dx_wide"), bf16_single());
  const int v[CTCN_DX_PLAN_INTS] = {p.eligible, p.wide, p.tiles_wide, p.tiles_128};
  memcpy(out, v, sizeof(v));
  return CTCN_OK;
}
extern "C" int ctcn_gemm_dx(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, float beta, int precision, void *ws,
                            size_t ws_bytes, void *stream) {
  const GemmShape g = {0, 0, M, N, K, lda, ldb, ldc, precision, 0};
  if (const int rc = check_gemm_shape(g)) return rc;
  CTCN_REQUIRE(A && B && C, "ctcn_gemm_dx: null pointer");
  CTCN_REQUIRE(!ws || (uintptr_t)ws % 16 == 0, "ctcn_gemm_dx: the workspace must be 16-byte aligned");
  const DxPlan p = plan_dx(M, N, K, lda, precision, (int)((uintptr_t)A & 15), ws != nullptr, ws_bytes, ctcn_device_cus(), ctcn_get_option("gemm_dx_wide"),
                           bf16_single());
  if (!p.wide) return gemm_core(0, 0, M, N, K, A, lda, B, ldb, C, ldc, beta, precision, ws, ws_bytes, stream, 0u, nullptr, 0);
  hipStream_t st = (hipStream_t)stream;
  const PlaneLayout lay = plane_layout(0, N, K);               // B's planes alone: Bh | Bl at the workspace's start
  unsigned short *bh = (unsigned short *)ws, *bl = bh + lay.b_el;
  launch_split(SP_TRANSPOSE, st, B, ldb, N, K, lay.Kp, bh, bl, 0, 0u, nullptr);
  CTCN_LAUNCH_CHECK();
  const size_t lds = (size_t)2 * (2 * 256 * 64 + 2 * 320 * 64);
  CTCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_af32_n320pp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(gemm_af32_n320pp_kernel, dim3(p.tiles_wide), dim3(512), lds, st, M, N, K, lay.Kp, A, lda, (const unsigned short *)bh,
                     (const unsigned short *)bl, C, ldc, beta, ceil_div(M, 256), N / 320);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

// the same transposition of two equally shaped tensors in ONE launch (W_hh of the two directions before a backward recurrence)
__global__ void transpose01_pair_kernel(const float *__restrict__ in0, const float *__restrict__ in1, float *__restrict__ out0, float *__restrict__ out1,
                                        int A, int B, int C) {
  const float *in = blockIdx.y ? in1 : in0;
  float *out = blockIdx.y ? out1 : out0;
  const size_t total = (size_t)A * B * C;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = i % C;
    const size_t ab = i / C;
    const int a = ab % A;
    const int b = ab / A;
    out[i] = in[((size_t)a * B + b) * C + c];
  }
}
// C == 1: a plain matrix transpose, out[b][a] = in[a][b], through a 32 x 33 LDS tile (both sides coalesced: 8.6 -> ~3 us for the
// two 1 280 x 320 W_hh of a cfg2 layer)
__global__ __launch_bounds__(256) void transpose2d_pair_kernel(const float *__restrict__ in0, const float *__restrict__ in1, float *__restrict__ out0,
                                                               float *__restrict__ out1, int A, int B) {
  __shared__ float tile[32][33];
  const float *in = blockIdx.z ? in1 : in0;
  float *out = blockIdx.z ? out1 : out0;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
  const int b0 = blockIdx.x * 32, a0 = blockIdx.y * 32;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int a = a0 + ty + 8 * k, b = b0 + tx;
    if (a < A && b < B) tile[ty + 8 * k][tx] = in[(size_t)a * B + b];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int b = b0 + ty + 8 * k, a = a0 + tx;
    if (a < A && b < B) out[(size_t)b * A + a] = tile[tx][ty + 8 * k];
  }
}
int ctcn_transpose01_pair(const float *in0, const float *in1, float *out0, float *out1, int A, int B, int C, void *stream) {
  CTCN_REQUIRE(in0 && in1 && out0 && out1 && A > 0 && B > 0 && C > 0, "ctcn_transpose01_pair: bad args");
  if (C == 1) {
    hipLaunchKernelGGL(transpose2d_pair_kernel, dim3(ceil_div(B, 32), ceil_div(A, 32), 2), dim3(256), 0, (hipStream_t)stream, in0, in1, out0, out1, A, B);
    CTCN_LAUNCH_CHECK();
    return CTCN_OK;
  }
  const size_t total = (size_t)A * B * C;
  const int blocks = (int)min((size_t)4096, ceil_div_z(total, 256));
  hipLaunchKernelGGL(transpose01_pair_kernel, dim3(blocks, 2), dim3(256), 0, (hipStream_t)stream, in0, in1, out0, out1, A, B, C);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}

extern "C" int ctcn_transpose01(const float *in, float *out, int A, int B, int C, void *stream) {
  CTCN_REQUIRE(in && out && A > 0 && B > 0 && C > 0, "ctcn_transpose01: bad args");
  const size_t total = (size_t)A * B * C;
  const int blocks = (int)min((size_t)4096, ceil_div_z(total, 256));
  hipLaunchKernelGGL(transpose01_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in, out, A, B, C);
  CTCN_LAUNCH_CHECK();
  return CTCN_OK;
}
