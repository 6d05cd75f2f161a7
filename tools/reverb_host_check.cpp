// reverb_host_check -- the host entry points of reverb.hip (ctcn_reverb_bank_bytes, ctcn_reverb_bank, ctcn_reverb_plan, ctcn_reverb_ws_bytes,
// ctcn_reverb_host) in a stand-alone program for a sanitizer run: every buffer is a heap block of exactly the size the contract asks for, so
// a read or write one element outside it is an error report, and the integer arithmetic of the draws runs under UBSan.  No device is used.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/reverb_host_check.cpp -o reverb_host_check && ./reverb_host_check
//
// Grid: banks of (R, N) in {(2, 2), (1, 0), (0, 1)} with impulse responses of 1, 37 and 1030 taps (peaks at 0, K - 1 and inside) and noises
// of 1, 7 and 3000 samples (one all zero), row strides equal to the longest row; n in {0, 1, 2, 1023, 1024, 1025, 2049}; int16 and float32;
// probabilities {0, 0.5, 1}^2; normalize on and off; 5 (seed, utterance index) pairs, high bits set among them.  Checked besides: the draws
// inside their ranges, finite output, both parts off equal to the input, the refusals' codes.
#include <cstdio>
#include <cstdlib>

#include "../ctc_pytorch_amd/csrc/reverb.hip"

static char last_error[512];
void ctcn_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof(last_error), fmt, ap);
  va_end(ap);
}

#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, last_error); \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)

static uint32_t lcg = 12345u;
static float noise_value() {
  lcg = lcg * 1664525u + 1013904223u;
  return (float)((int)(lcg >> 16) - 32768) / 64.f;
}

int main() {
  const int rir_len[3] = {1030, 37, 1}, rir_peak[3] = {400, 36, 0}, noise_len[3] = {7, 3000, 1};
  const int shapes[3][2] = {{2, 2}, {1, 0}, {0, 1}};
  const uint64_t keys[5][2] = {{0, 0}, {5, 1}, {0xFEDCBA9876543210ull, 7}, {~0ull, 1ull << 55}, {2019, (1ull << 32) + 3}};
  const float probs[3] = {0.f, 0.5f, 1.f};
  const double snrs[3] = {20.0, 0.0, -5.0};
  long long calls = 0;
  for (int si = 0; si < 3; ++si)
    for (int first = 0; first < 2; ++first) {                             // which rows of the tables above the bank starts from
      const int R = shapes[si][0], N = shapes[si][1];
      int kstride = 0, lstride = 0;
      for (int r = 0; r < R; ++r) kstride = std::max(kstride, rir_len[first + r]);
      for (int m = 0; m < N; ++m) lstride = std::max(lstride, noise_len[first + m]);
      float *h = (float *)malloc(sizeof(float) * (size_t)std::max(R * kstride, 1)), *q = (float *)malloc(sizeof(float) * (size_t)std::max(N * lstride, 1));
      int32_t *hl = (int32_t *)malloc(sizeof(int32_t) * (size_t)std::max(R, 1)), *ql = (int32_t *)malloc(sizeof(int32_t) * (size_t)std::max(N, 1));
      for (int r = 0; r < R; ++r) {
        hl[r] = rir_len[first + r];
        for (int k = 0; k < kstride; ++k) h[r * kstride + k] = k < hl[r] ? noise_value() / 2000.f : NAN;
        h[r * kstride + std::min(rir_peak[first + r], hl[r] - 1)] = 1.f;
      }
      for (int m = 0; m < N; ++m) {
        ql[m] = noise_len[first + m];
        for (int i = 0; i < lstride; ++i) q[m * lstride + i] = i < ql[m] ? (ql[m] == 1 ? 0.f : noise_value()) : NAN;
      }
      const int J = N ? 3 : 0;
      const size_t bytes = ctcn_reverb_bank_bytes(R, kstride, N, lstride, J);
      EXPECT(bytes > 0);
      void *bank = malloc(bytes);
      EXPECT(ctcn_reverb_bank(R ? h : nullptr, R ? hl : nullptr, R, kstride, N ? q : nullptr, N ? ql : nullptr, N, lstride, J ? snrs : nullptr, J, 1000.0, bank,
                              bytes) == CTCN_OK);
      EXPECT(ctcn_reverb_bank(R ? h : nullptr, R ? hl : nullptr, R, kstride, N ? q : nullptr, N ? ql : nullptr, N, lstride, J ? snrs : nullptr, J, 1000.0, bank,
                              bytes - 4) == CTCN_EINVAL);
      EXPECT(ctcn_reverb_ws_bytes(bank, 3, 2049) > 0 && ctcn_reverb_ws_bytes(bank, 0, 2049) == 0);
      for (int n : {0, 1, 2, 1023, 1024, 1025, 2049})
        for (int i16 = 0; i16 < 2; ++i16) {
          void *x = malloc((size_t)std::max(n, 1) * (i16 ? 2 : 4));
          float *out = (float *)malloc(sizeof(float) * (size_t)std::max(n, 1));
          for (int i = 0; i < n; ++i) {
            if (i16) ((int16_t *)x)[i] = (int16_t)(noise_value() * 32.f);
            else ((float *)x)[i] = noise_value();
          }
          for (float pr : probs)
            for (float pn : probs)
              for (int normalize = 0; normalize < 2; ++normalize)
                for (const uint64_t *k : keys) {
                  ctcn_reverb_opts o = {pr, pn, normalize};
                  int32_t d[4];
                  EXPECT(ctcn_reverb_plan(bank, &o, k[0], k[1], d) == CTCN_OK);
                  EXPECT(d[0] >= -1 && d[0] < R && d[1] >= -1 && d[1] < N);
                  if (d[1] >= 0) EXPECT(d[2] >= 0 && d[2] < J && d[3] >= 0 && d[3] < ql[d[1]]);
                  if (pr == 0.f) EXPECT(d[0] == -1);
                  if (pn == 0.f) EXPECT(d[1] == -1);
                  if (pr == 1.f && R) EXPECT(d[0] >= 0);
                  EXPECT(ctcn_reverb_host(n ? x : nullptr, i16, n, bank, &o, k[0], k[1], n ? out : nullptr) == CTCN_OK);
                  ++calls;
                  for (int i = 0; i < n; ++i) {
                    EXPECT(std::isfinite(out[i]));
                    if (d[0] < 0 && d[1] < 0) EXPECT(out[i] == (i16 ? (float)((int16_t *)x)[i] : ((float *)x)[i]));
                  }
                }
          free(x);
          free(out);
        }
      free(bank); free(h); free(q); free(hl); free(ql);
    }
  // refusals
  float one[4] = {1.f, 0.5f, 0.25f, 0.f}, two[4];
  int32_t len4 = 4, len0 = 0, d[4];
  double snr17[17] = {0}, bad_snr = NAN;
  alignas(8) char block[4096];
  EXPECT(ctcn_reverb_bank_bytes(0, 0, 0, 0, 0) == 0 && ctcn_reverb_bank_bytes(1, 16385, 0, 0, 0) == 0 && ctcn_reverb_bank_bytes(0, 0, 1, 4, 17) == 0);
  EXPECT(ctcn_reverb_bank(one, &len4, 1, 16385, nullptr, nullptr, 0, 0, nullptr, 0, 16000.0, block, sizeof(block)) == CTCN_EUNSUPPORTED);
  EXPECT(ctcn_reverb_bank(nullptr, nullptr, 0, 0, one, &len4, 1, 4, snr17, 17, 16000.0, block, sizeof(block)) == CTCN_EUNSUPPORTED);
  EXPECT(ctcn_reverb_bank(one, &len0, 1, 4, nullptr, nullptr, 0, 0, nullptr, 0, 16000.0, block, sizeof(block)) == CTCN_EINVAL);
  EXPECT(ctcn_reverb_bank(nullptr, nullptr, 0, 0, one, &len4, 1, 4, &bad_snr, 1, 16000.0, block, sizeof(block)) == CTCN_EINVAL);
  EXPECT(ctcn_reverb_bank(one, &len4, 1, 4, nullptr, nullptr, 0, 0, nullptr, 0, 16000.0, block, sizeof(block)) == CTCN_OK);
  ctcn_reverb_opts bad = {1.5f, 0.f, 1}, nan_p = {0.f, NAN, 1}, ok = {1.f, 1.f, 1};
  EXPECT(ctcn_reverb_plan(block, &bad, 1, 0, d) == CTCN_EINVAL && ctcn_reverb_host(one, 0, 4, block, &nan_p, 1, 0, two) == CTCN_EINVAL);
  EXPECT(ctcn_reverb_host(one, 0, 4, block, &ok, 1, 0, one) == CTCN_EINVAL && ctcn_reverb_host(one, 0, 4, one, &ok, 1, 0, two) == CTCN_EINVAL);
  EXPECT(ctcn_reverb_host(one, 0, 4, block, &ok, 1, 0, two) == CTCN_OK && ctcn_reverb_limits(nullptr) == CTCN_EINVAL);
  printf("reverb_host_check: %lld calls of ctcn_reverb_host, no finding\n", calls);
  return 0;
}
