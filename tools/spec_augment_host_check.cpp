// spec_augment_host_check -- the host entry points of specaug.hip (ctcn_spec_augment_plan, ctcn_spec_augment_host) in a stand-alone program
// for a sanitizer run: every buffer is a heap block of exactly the size the contract asks for, so a read or write one element outside it
// is an error report, and the int64 / uint64 arithmetic of the draws runs under UBSan.  No device is used.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/spec_augment_host_check.cpp -o spec_augment_host_check && ./spec_augment_host_check
//
// Grid: T in 0..70 x F in {1, 5, 81} x warp_window in {0, 1, 6, 40} x (frequency masks, width) in {0,0 1,3 8,200} x (time masks, width, ratio)
// in {0,0,1 2,10,0.5 32,1000,1} x 6 (seed, utterance index) pairs, high bits set among them.  Checked besides: every interval inside its
// axis, the warp's c and w inside their ranges, masked elements equal to fill, everything off equal to the input, the refusals' codes.
#include <cstdio>
#include <cstdlib>

#include "../ctc_pytorch_amd/csrc/specaug.hip"

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

int main() {
  const int windows[4] = {0, 1, 6, 40}, fm[3][2] = {{0, 0}, {1, 3}, {8, 200}}, tm[3][2] = {{0, 0}, {2, 10}, {32, 1000}};
  const float ratios[3] = {1.f, 0.5f, 1.f};
  const uint64_t keys[6][2] = {{0, 0}, {5, 1}, {0xFEDCBA9876543210ull, 7}, {1, 0xFFFFFFFFFFFFFFFFull}, {~0ull, 1ull << 56}, {2019, (1ull << 32) + 3}};
  const float fill = -1.5f;
  long long calls = 0;
  for (int F : {1, 5, 81})
    for (int W : windows)
      for (int fi = 0; fi < 3; ++fi)
        for (int ti = 0; ti < 3; ++ti) {
          ctcn_specaug_opts o = {W, fm[fi][0], fm[fi][1], tm[ti][0], tm[ti][1], ratios[ti], fill};
          const bool off = W == 0 && fi == 0 && ti == 0;
          for (int T = 0; T <= 70; ++T) {
            float *x = static_cast<float *>(malloc(sizeof(float) * (size_t)T * F + 1));
            float *out = static_cast<float *>(malloc(sizeof(float) * (size_t)T * F + 1));
            int32_t *warp = static_cast<int32_t *>(malloc(sizeof(int32_t) * 2));
            int32_t *freq = static_cast<int32_t *>(malloc(sizeof(int32_t) * 2 * o.num_freq_masks + 1));
            int32_t *time = static_cast<int32_t *>(malloc(sizeof(int32_t) * 2 * o.num_time_masks + 1));
            for (int i = 0; i < T * F; ++i) x[i] = (float)((i * 37) % 101) - 50.f;
            for (auto &k : keys) {
              EXPECT(ctcn_spec_augment_plan(&o, k[0], k[1], T, F, warp, freq, time) == CTCN_OK);
              if (W > 0 && T > 2 * W) EXPECT(warp[0] >= W && warp[0] < T - W && warp[1] >= 1 && warp[1] <= T - 1 && abs(warp[1] - warp[0]) < W);
              else EXPECT(warp[0] == 0 && warp[1] == 0);
              for (int m = 0; m < o.num_freq_masks; ++m)
                EXPECT(freq[2 * m] >= 0 && freq[2 * m + 1] >= 0 && freq[2 * m + 1] <= o.freq_width && freq[2 * m] + freq[2 * m + 1] <= F);
              for (int m = 0; m < o.num_time_masks; ++m)
                EXPECT(time[2 * m] >= 0 && time[2 * m + 1] >= 0 && time[2 * m + 1] <= o.time_width && time[2 * m + 1] <= (int)(o.time_ratio * T) &&
                       time[2 * m] + time[2 * m + 1] <= T);
              EXPECT(ctcn_spec_augment_host(x, T, F, &o, k[0], k[1], out) == CTCN_OK);
              ++calls;
              for (int m = 0; m < o.num_time_masks; ++m)
                for (int t = time[2 * m]; t < time[2 * m] + time[2 * m + 1]; ++t)
                  for (int f = 0; f < F; ++f) EXPECT(out[(size_t)t * F + f] == fill);
              for (int m = 0; m < o.num_freq_masks; ++m)
                for (int t = 0; t < T; ++t)
                  for (int f = freq[2 * m]; f < freq[2 * m] + freq[2 * m + 1]; ++f) EXPECT(out[(size_t)t * F + f] == fill);
              if (off)
                for (int i = 0; i < T * F; ++i) EXPECT(out[i] == x[i]);
            }
            free(time);
            free(freq);
            free(warp);
            free(out);
            free(x);
          }
        }
  float one[8] = {0}, two[8] = {0};
  int32_t iv[80];
  ctcn_specaug_opts bad = {0, 9, 1, 0, 0, 1.f, 0.f};
  EXPECT(ctcn_spec_augment_plan(&bad, 1, 0, 4, 2, iv, iv, iv) == CTCN_EUNSUPPORTED && ctcn_spec_augment_host(one, 4, 2, &bad, 1, 0, two) == CTCN_EUNSUPPORTED);
  ctcn_specaug_opts neg = {-1, 0, 0, 0, 0, 1.f, 0.f};
  EXPECT(ctcn_spec_augment_plan(&neg, 1, 0, 4, 2, iv, iv, iv) == CTCN_EINVAL && ctcn_spec_augment_host(one, 4, 2, &neg, 1, 0, two) == CTCN_EINVAL);
  ctcn_specaug_opts ok = {0, 0, 0, 0, 0, 1.f, 0.f};
  EXPECT(ctcn_spec_augment_host(one, 4, 2, &ok, 1, 0, one) == CTCN_EINVAL && ctcn_spec_augment_host(one, (1 << 30) + 1, 2, &ok, 1, 0, two) == CTCN_EINVAL);
  EXPECT(ctcn_spec_augment(one, nullptr, &ok, 1, 0, two, 1, 4, 2, nullptr) == CTCN_EINVAL);
  printf("spec_augment_host_check: %lld calls of ctcn_spec_augment_host, no finding\n", calls);
  return 0;
}
