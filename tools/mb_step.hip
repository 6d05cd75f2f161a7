// tools/mb_step.hip -- standalone micro-benchmark of the recurrent step kernels (development aid, not product).
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/mb_step.bin tools/mb_step.hip ctc_pytorch_amd/csrc/core.hip
#define CTCN_PERSIST_STATS 1
#include "../ctc_pytorch_amd/csrc/rnn.hip"
#include <vector>

extern "C" int ctcn_gemm(int, int, int, int, int, const float *, int, const float *, int, float *, int, float, int, void *, size_t, void *) { return 0; }
extern "C" int ctcn_transpose01(const float *, float *, int, int, int, void *) { return 0; }
int ctcn_transpose01_pair(const float *, const float *, float *, float *, int, int, int, void *) { return 0; }
extern "C" int ctcn_dropout(const float *, float *, size_t, float, uint64_t, uint64_t, void *) { return 0; }
int ctcn_gemm_on_xcds(int, int, int, int, int, const float *, int, const float *, int, float *, int, float, int, void *, size_t, void *, unsigned, GemmPlanes *) { return 0; }
int ctcn_gemm_shift_b(int, int, int, const float *, int, const float *, int, float *, int, float, int, void *, size_t, void *, unsigned, int, GemmPlanes *) { return 0; }
extern "C" int ctcn_gemm_dx(int, int, int, const float *, int, const float *, int, float *, int, float, int, void *, size_t, void *) { return 0; }

namespace {
__global__ void empty_kernel(RnnArgs p) { if (p.T < 0) p.y[0] = 1.f; }

// variant: matmul only (no epilogue global traffic)
template <int MT, int KQ4>
__global__ __launch_bounds__(256) void fwd_mm_only(RnnArgs p) {
  constexpr int NW = 4;
  __shared__ float red[NW * MT * 256];
  __shared__ float outs[MT * 16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int d = blockIdx.y, H = p.H, D = p.D, B = p.B;
  const int t = d == 0 ? p.step : p.T - 1 - p.step, tp = d == 0 ? t - 1 : t + 1;
  const int j0 = blockIdx.x * 4, gate = r >> 2, jj = r & 3;
  const float *W = d == 0 ? p.w0 : p.w1;
  const float *brow = W + (size_t)(gate * H + j0 + jj) * H;
  f32x4 acc[MT];
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float *abase = p.y + ((size_t)tp * B) * D * H + d * H;
  rec_mm<MT, KQ4>(abase, D * H, H, abase, D * H, B, brow, true, H, NW, wave, q, r, acc);
  reduce_tiles<MT, NW, 4>(acc, red, outs, tid, 256);
  if (tid < 128 && outs[tid >> 2][tid & 3] == 12345.f) p.y[0] = 1.f;
}
// variant: loads only (no MFMA): sum the operands
template <int MT, int KQ4>
__global__ __launch_bounds__(256) void fwd_ld_only(RnnArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int d = blockIdx.y, H = p.H, D = p.D, B = p.B;
  const int t = d == 0 ? p.step : p.T - 1 - p.step, tp = d == 0 ? t - 1 : t + 1;
  const int j0 = blockIdx.x * 4, gate = r >> 2, jj = r & 3;
  const float *W = d == 0 ? p.w0 : p.w1;
  const float *brow = W + (size_t)(gate * H + j0 + jj) * H;
  const float *abase = p.y + ((size_t)tp * B) * D * H + d * H;
  float s = 0.f;
  const int kb = wave * 16 * KQ4 + q * 4;
  float4 v[KQ4 * (MT + 1)];
  for (int i = 0; i < KQ4; ++i) {
    v[i] = *(const float4 *)(brow + kb + 16 * i);
    for (int mt = 0; mt < MT; ++mt) v[KQ4 * (1 + mt) + i] = *(const float4 *)(abase + (size_t)(mt * 16 + r) * D * H + kb + 16 * i);
  }
  for (int i = 0; i < KQ4 * (MT + 1); ++i) s += v[i].x + v[i].y + v[i].z + v[i].w;
  if (s == 12345.f) p.y[0] = 1.f;
}

// instrumented copy of rnn_fwd_step<2,5> (LSTM): wall_clock64 stamps (100 MHz -> 10 ns) of block 0 / wave 0
__global__ __launch_bounds__(256) void fwd_stamped(RnnArgs p, long long *stamps) {
  constexpr int NW = 4, MT = 2, KQ4 = 5;
  __shared__ float red[NW * MT * 256];
  __shared__ float outs[MT * 16][17];
  long long ts[8];
  ts[0] = clock64();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int d = blockIdx.y, b0 = 0, H = p.H, G = p.G, D = p.D, B = p.B, Bc = 32;
  const int t = d == 0 ? p.step : p.T - 1 - p.step, tp = d == 0 ? t - 1 : t + 1;
  const int j0 = blockIdx.x * 4, gate = r >> 2, jj = r & 3;
  const float *W = d == 0 ? p.w0 : p.w1;
  const float *brow = W + (size_t)(gate * H + j0 + jj) * H;
  const int bl = tid / 4, jl = tid - bl * 4, j = j0 + jl, b = b0 + bl;
  const bool item = bl < Bc;
  const size_t row_t = (size_t)t * B + b;
  float pre[4] = {0, 0, 0, 0}, prev = 0;
  if (item) {
    const float *gt = p.gates + (row_t * D + d) * (size_t)(G * H);
    for (int k = 0; k < 4; ++k) pre[k] = gt[k * H + j];
    prev = p.aux[(((size_t)tp * B + b) * D + d) * H + j];
  }
  f32x4 acc[MT];
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float *abase = p.y + ((size_t)tp * B + b0) * D * H + d * H;
  ts[1] = clock64();
  rec_mm<MT, KQ4>(abase, D * H, H, abase, D * H, Bc, brow, true, H, NW, wave, q, r, acc);
  asm volatile("" :: "v"(acc[0][0]), "v"(acc[1][0]));
  ts[2] = clock64();
  reduce_tiles<MT, NW, 4>(acc, red, outs, tid, 256);
  ts[3] = clock64();
  float hv = 0;
  if (item) {
    float *gt = p.gates + (row_t * D + d) * (size_t)(G * H);
    float *yt = p.y + row_t * D * H + d * H;
    const float i_ = sigmoidf_(outs[bl][0 * 4 + jl] + pre[0]);
    const float f_ = sigmoidf_(outs[bl][1 * 4 + jl] + pre[1]);
    const float g_ = tanhf(outs[bl][2 * 4 + jl] + pre[2]);
    const float o_ = sigmoidf_(outs[bl][3 * 4 + jl] + pre[3]);
    const float c = f_ * prev + i_ * g_;
    hv = o_ * tanhf(c);
    asm volatile("" :: "v"(hv));
    ts[4] = clock64();
    gt[0 * H + j] = i_; gt[1 * H + j] = f_; gt[2 * H + j] = g_; gt[3 * H + j] = o_;
    p.aux[(row_t * D + d) * H + j] = c;
    yt[j] = hv;
  }
  ts[5] = clock64();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ts[6] = clock64();
  if (blockIdx.x == 7 && blockIdx.y == 0 && tid == 0 && p.step == 400)
    for (int i = 0; i < 7; ++i) stamps[i] = ts[i] - ts[0];
}
}  // namespace

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

int main() {
  const int T = 800, B = 32, H = 320, D = 2, G = 4;
  float *y, *gates, *aux, *w, *wT, *dy, *state;
  CK(hipMalloc(&y, (size_t)T * B * D * H * 4)); CK(hipMalloc(&gates, (size_t)T * B * D * G * H * 4)); CK(hipMalloc(&aux, (size_t)T * B * D * H * 4));
  CK(hipMalloc(&w, (size_t)D * G * H * H * 4)); CK(hipMalloc(&wT, (size_t)D * G * H * H * 4)); CK(hipMalloc(&dy, (size_t)T * B * D * H * 4));
  CK(hipMalloc(&state, (size_t)B * D * H * 4));
  CK(hipMemset(y, 0, (size_t)T * B * D * H * 4)); CK(hipMemset(gates, 0, (size_t)T * B * D * G * H * 4)); CK(hipMemset(aux, 0, (size_t)T * B * D * H * 4));
  CK(hipMemset(w, 0, (size_t)D * G * H * H * 4)); CK(hipMemset(wT, 0, (size_t)D * G * H * H * 4)); CK(hipMemset(dy, 0, (size_t)T * B * D * H * 4));
  CK(hipMemset(state, 0, (size_t)B * D * H * 4));
  RnnArgs a; a.cell = 0; a.T = T; a.B = B; a.H = H; a.D = D; a.G = G; a.step = 0; a.w0 = w; a.w1 = w + (size_t)G * H * H; a.y = y; a.gates = gates;
  a.aux = aux; a.dy = dy; a.state = state;
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto timeit = [&](const char *name, auto launch, int s0) {
    for (int rep = 0; rep < 2; ++rep) {
      hipEventRecord(e0, st);
      for (int s = s0; s < T; ++s) { a.step = s; launch(); }
      hipEventRecord(e1, st);
      hipEventSynchronize(e1);
    }
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-44s %8.2f us/step\n", name, ms * 1e3 / (T - s0));
    return 0;
  };
  dim3 gf(H / 4, D, 1), gb(H / 16, D, 2);
  timeit("empty 160x256", [&] { hipLaunchKernelGGL(empty_kernel, gf, dim3(256), 0, st, a); }, 1);
  timeit("empty 80x1024", [&] { hipLaunchKernelGGL(empty_kernel, gb, dim3(1024), 0, st, a); }, 1);
  timeit("fwd full <2,5>", [&] { hipLaunchKernelGGL((rnn_fwd_step<2, 5>), gf, dim3(256), 0, st, a); }, 1);
  timeit("fwd loads only", [&] { hipLaunchKernelGGL((fwd_ld_only<2, 5>), gf, dim3(256), 0, st, a); }, 1);
  timeit("fwd matmul+reduce only", [&] { hipLaunchKernelGGL((fwd_mm_only<2, 5>), gf, dim3(256), 0, st, a); }, 1);
  a.w0 = wT; a.w1 = wT + (size_t)G * H * H;
  timeit("bwd full <5> 80x1024", [&] { hipLaunchKernelGGL((rnn_bwd_step<5>), gb, dim3(1024), 0, st, a); }, 1);
  {
    long long *stamps, h[8];
    CK(hipMalloc(&stamps, 64)); CK(hipMemset(stamps, 0, 64));
    timeit("fwd stamped <2,5>", [&] { hipLaunchKernelGGL(fwd_stamped, gf, dim3(256), 0, st, a, stamps); }, 1);
    CK(hipMemcpy(h, stamps, 56, hipMemcpyDeviceToHost));
    printf("  stamps (shader cycles since kernel entry, block 7 wave 0, step 400): prefetch-issued %lld | matmul-done %lld | reduce-done %lld | math-done %lld | stores-issued %lld | stores-acked %lld\n",
           h[1], h[2], h[3], h[4], h[5], h[6]);
  }
  {
    // persistent forward / backward recurrences with in-kernel phase accounting (forward), device-scope vs XCD-local
    const int nbt = 2, K = G * H;
    const size_t hx_bytes = (size_t)2 * D * nbt * 32 * 32 * 1024, fl_bytes = (size_t)2 * D * nbt * 32 * 32 * 4 + 256;
    float *hx; unsigned *flags; int *status; long long *stats, h[16 + 64 * 12];   // records of rnn.hip's Stamps::report: the kernel's phases in the order of its enum, total cycles, HW_ID
    CK(hipMalloc(&hx, hx_bytes)); CK(hipMalloc(&flags, fl_bytes)); CK(hipMalloc(&status, 4)); CK(hipMalloc(&stats, sizeof(h))); CK(hipMemset(stats, 0, sizeof(h)));
    const int nx = ctcn_device_xcds();
    printf("device XCDs (even deal verified): %d\n", nx);
    struct Cfg { int local, hsu, nt, prec, pd; } cfgs[] = {{1, 8, 2, 1, 2}, {1, 12, 3, 1, 2}, {1, 16, 4, 1, 2}};   // measured besides: HSU 4 -> 2.55, HSU 10 (4-B publish pieces) -> 2.37, polls 1 / 3 / 4 -> 2.08 / 2.09 / 2.15 us
    for (auto &c : cfgs) {
      if (c.local && nx <= 1) continue;
      PersistArgs pa = {}; pa.a = a; pa.a.w0 = w; pa.a.w1 = w + (size_t)G * H * H; pa.hx = hx; pa.flags = flags; pa.status = status; pa.spin_limit = 1 << 20; pa.stats = stats;
      pa.poll_delay = 0; pa.poll_depth = c.pd; pa.local = c.local; pa.nx = c.local ? nx : 1; pa.nbt = nbt; pa.hsu = c.hsu; pa.nsl = (H + c.hsu - 1) / c.hsu;
      const int wpx = (D * nbt + pa.nx - 1) / pa.nx * pa.nsl;
      pa.wpx = wpx; pa.tickets = flags + (fl_bytes - 256) / 4;
      dim3 gp = c.local ? dim3(pa.nx * (wpx + 4), 1, 1) : dim3(pa.nsl, D, nbt);
      const size_t lds = 0;
      for (int rep = 0; rep < 2; ++rep) {
        CK(hipMemsetAsync(flags, 0, fl_bytes, st)); CK(hipMemsetAsync(status, 0, 4, st));
        hipEventRecord(e0, st);
        if (c.prec) CK(hipMemsetAsync(hx, 0, hx_bytes, st));
        if (c.nt == 2 && !c.prec) hipLaunchKernelGGL((rnn_fwd_persist<2, 5, 0, 0>), gp, dim3(256), lds, st, pa);
        else if (c.nt == 3 && !c.prec) hipLaunchKernelGGL((rnn_fwd_persist<3, 5, 0, 0>), gp, dim3(256), lds, st, pa);
        else if (c.nt == 2) hipLaunchKernelGGL((rnn_fwd_persist<2, 5, 1, 0>), gp, dim3(256), lds, st, pa);
        else if (c.nt == 1) hipLaunchKernelGGL((rnn_fwd_persist<1, 5, 1, 0>), gp, dim3(256), lds, st, pa);
        else if (c.nt == 3) hipLaunchKernelGGL((rnn_fwd_persist<3, 5, 1, 0>), gp, dim3(256), lds, st, pa);
        else hipLaunchKernelGGL((rnn_fwd_persist<4, 5, 1, 0>), gp, dim3(256), lds, st, pa);
        hipEventRecord(e1, st); hipEventSynchronize(e1);
      }
      float ms; hipEventElapsedTime(&ms, e0, e1);
      int hs = -1; CK(hipMemcpy(&hs, status, 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h, stats, sizeof(h), hipMemcpyDeviceToHost));
      printf("fwd PERSISTENT local=%d HSU=%2d NT=%d precision=%d polls=%d  %3d slices/group   %8.2f us/step   (status %d)\n", c.local, c.hsu, c.nt, c.prec, c.pd, pa.nsl, ms * 1e3 / T, hs);
      // rnn_fwd_persist: poll, fill, mm, red, sum, math, hpub, pub, drain, tail | total | HW_ID; item wave 0 of slice 7 at 0, the communication wave of slice k at 16 + 12 k
      const long long *cw = h + 16 + 12 * 7;
      const long long wait_math = cw[4] + cw[5] + cw[6];
      printf("  per step (cycles), slice 7, communication wave: flag poll+barrier %.0f | operand loads %.0f | mfma %.0f | reduce %.0f | gate math+publish %.0f | total %.0f\n",
             (double)cw[0] / T, (double)cw[1] / T, (double)cw[2] / T, (double)cw[3] / T, (double)(wait_math + cw[7] + cw[8] + cw[9]) / T, (double)cw[10] / T);
      if (c.local) {
        printf("    per slice: poll / rest cycles per step [se.sh.cu]:");
        for (int i = 0; i < pa.nsl; ++i) {
          const long long *r = h + 16 + 12 * i;
          const unsigned hw = (unsigned)r[11];
          long long rest = 0;
          for (int k = 1; k < 10; ++k) rest += r[k];
          printf(" %d:%.0f/%.0f[%u.%u.%u]", i, (double)r[0] / T, (double)rest / T, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15);
        }
        printf("\n");
      }
      printf("    gate math+publish split: wait for gate math (hpub barrier) %.0f | convert + issue stores %.0f | drain %.0f | flag + tail %.0f\n",
             (double)wait_math / T, (double)cw[7] / T, (double)cw[8] / T, (double)cw[9] / T);
      printf("    item wave 0: partial sums (4 x 16-B LDS reads) %.0f | gate math + split + hpub writes %.0f\n", (double)h[4] / T, (double)h[5] / T);
    }
    for (int pd : {0, 8}) {   // tagged-gather forward (round 2): 64-cycle sleeps before the first poll of a step
      if (nx <= 1) break;
      PersistArgs pa = {}; pa.a = a; pa.a.w0 = w; pa.a.w1 = w + (size_t)G * H * H; pa.hx = hx; pa.flags = flags; pa.status = status; pa.spin_limit = 1 << 20; pa.stats = stats;
      pa.poll_depth = 1; pa.poll_delay = pd; pa.local = 1; pa.nx = nx; pa.nbt = nbt; pa.hsu = 16; pa.nsl = H / 16; pa.tagmode = 1;
      const int wpx = (D * nbt + pa.nx - 1) / pa.nx * pa.nsl;
      pa.wpx = wpx; pa.tickets = flags + (fl_bytes - 256) / 4;
      dim3 gp = dim3(pa.nx * (wpx + 4), 1, 1);
      for (int rep = 0; rep < 2; ++rep) {
        CK(hipMemsetAsync(flags, 0, fl_bytes, st)); CK(hipMemsetAsync(status, 0, 4, st)); CK(hipMemsetAsync(hx, 0, hx_bytes, st));
        hipEventRecord(e0, st);
        hipLaunchKernelGGL((rnn_fwd_tagged<1, 0>), gp, dim3(1024), 0, st, pa);
        hipEventRecord(e1, st); hipEventSynchronize(e1);
      }
      float ms; hipEventElapsedTime(&ms, e0, e1);
      int hs = -1; CK(hipMemcpy(&hs, status, 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h, stats, sizeof(h), hipMemcpyDeviceToHost));
      printf("fwd TAGGED GATHER poll delay=%d  %3d slices/group   %8.2f us/step   (status %d)\n", pd, pa.nsl, ms * 1e3 / T, hs);
      printf("  per step (cycles), slice 3, exchange wave 4: poll until the block is valid %.0f | perm + 12 mfma + park %.0f | barrier wait %.0f | total %.0f   [%.2f full polls per step, %.0f cycles per poll round trip]\n",
             (double)(h[0] + h[1]) / T, (double)h[2] / T, (double)h[3] / T, (double)h[9] / T, (double)h[8] / T, (double)h[1] / (double)(h[8] ? h[8] : 1));
      // (rnn_fwd_tagged: idle, poll, mm, barrier, sum, math, pub, rsv, polls | total; exchange wave 4 of slice 3 at 0, item wave 0 at 16)
      printf("  item wave 0: wait for the barrier %.0f | 12 partial reads + sums %.0f | gate math %.0f | split + publish issue %.0f | reserve issue %.0f\n",
             (double)h[16 + 3] / T, (double)h[16 + 4] / T, (double)h[16 + 5] / T, (double)h[16 + 6] / T, (double)h[16 + 7] / T);
    }
    for (int lp = 0; lp < 3; ++lp) {
      const int local = 1, prec = 1, pd = 2, scatter = lp, bdelay = 0;
      if (nx <= 1) continue;
      PersistArgs pa = {}; pa.a = a; pa.a.w0 = wT; pa.a.w1 = wT + (size_t)G * H * H; pa.hx = hx; pa.flags = flags; pa.status = status; pa.spin_limit = 1 << 20; pa.stats = stats;
      pa.poll_depth = pd; pa.poll_delay = bdelay; pa.local = local; pa.nx = nx; pa.nbt = nbt; pa.hsu = 16; pa.nsl = (H + 15) / 16;
      const int wpx = (D * nbt + pa.nx - 1) / pa.nx * pa.nsl;
      pa.wpx = wpx; pa.tickets = flags + (fl_bytes - 256) / 4;
      dim3 gp = dim3(pa.nx * (wpx + 4), 1, 1);
      for (int rep = 0; rep < 2; ++rep) {
        CK(hipMemsetAsync(flags, 0, fl_bytes, st)); CK(hipMemsetAsync(status, 0, 4, st)); CK(hipMemsetAsync(hx, 0, hx_bytes, st));
        hipEventRecord(e0, st);
        pa.tagmode = scatter == 2;
        if (scatter == 2) hipLaunchKernelGGL((rnn_bwd_scatter<2, 1, true, 0>), gp, dim3(1024), 0, st, pa);
        else if (scatter) hipLaunchKernelGGL((rnn_bwd_scatter<2, 1, false, 0>), gp, dim3(1024), 0, st, pa);
        else hipLaunchKernelGGL((rnn_bwd_persist<5, 1>), gp, dim3(1024), 0, st, pa);
        hipEventRecord(e1, st); hipEventSynchronize(e1);
      }
      float ms; hipEventElapsedTime(&ms, e0, e1);
      int hs = -1; CK(hipMemcpy(&hs, status, 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(h, stats, sizeof(h), hipMemcpyDeviceToHost));
      // rnn_bwd_persist: poll, mm, red, math, copy, tail | total, wave 0 at 0, wave 15 at 8;  rnn_bwd_scatter: gather, sum, math, staged, scatter, drain, tail | total, at 0 and 16
      for (int wv = 0; wv < 2; ++wv) {
        const long long *r = h + wv * (scatter ? 16 : 8);
        const long long col[7] = {r[0], scatter ? 0 : r[1], scatter ? r[1] + r[2] + r[3] : r[2], scatter ? r[4] : r[3], scatter ? r[5] : r[4], scatter ? r[6] : r[5], scatter ? r[7] : r[6]};
        printf("  bwd %s per step (cycles), slice 3, %s: %s %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | total %.0f\n", scatter == 2 ? "SCATTER tagged" : scatter ? "SCATTER flags" : "gather",
               wv ? "wave 15 (exchange)" : "wave 0 (items)", scatter ? "gather+park+barrier | - | item sum+math+stage+barrier | lds+mfma+scatter issue | drain+flags | reserve traffic:" : "phases:",
               (double)col[0] / T, (double)col[1] / T, (double)col[2] / T, (double)col[3] / T, (double)col[4] / T, (double)col[5] / T, (double)col[6] / T);
      }
      if (scatter) printf("    item wave, inside 'item sum+math+stage+barrier': partial sum (12 LDS reads) %.0f | gate math + stage writes %.0f | barrier wait %.0f\n",
                          (double)h[1] / T, (double)h[2] / T, (double)h[3] / T);
      printf("bwd PERSISTENT %s delay %d  %8.2f us/step   (status %d)\n", scatter == 2 ? "scatter tagged" : scatter ? "scatter flags" : "gather", bdelay, ms * 1e3 / T, hs);
    }
  }
  // graph replay of the forward loop: is the host the limiter?
  a.w0 = w; a.w1 = w + (size_t)G * H * H;
  hipGraph_t g; hipGraphExec_t ge;
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
  for (int s = 1; s < T; ++s) { a.step = s; hipLaunchKernelGGL((rnn_fwd_step<2, 5>), gf, dim3(256), 0, st, a); }
  CK(hipStreamEndCapture(st, &g));
  CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  for (int rep = 0; rep < 2; ++rep) { hipEventRecord(e0, st); CK(hipGraphLaunch(ge, st)); hipEventRecord(e1, st); hipEventSynchronize(e1); }
  float ms; hipEventElapsedTime(&ms, e0, e1);
  printf("%-44s %8.2f us/step\n", "fwd full <2,5> hipGraph replay", ms * 1e3 / (T - 1));
  return 0;
}
