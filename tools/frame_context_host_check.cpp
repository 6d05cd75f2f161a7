// frame_context_host_check -- the host entry points of context.hip (ctcn_context_frames, ctcn_delta_scales, ctcn_frame_context_tile,
// ctcn_frame_context_host) in a stand-alone program for a sanitizer run: every buffer is a heap block of exactly the size the contract asks
// for, so a read or write one element outside it is an error report.  No device is used.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/frame_context_host_check.cpp -o frame_context_host_check && ./frame_context_host_check
//
// Grid: T in 0..40 x F in {1, 5} x (left, right) in {0,0 0,2 3,3 5,5} x skip in {0,1,2,3,7} x n_downsample in {1,2,4} x delta order 0..2 x
// window in {1,2,5}, with the output buffer at n_out rows and at n_out + 3.  Checked besides: the return value against ctcn_context_frames,
// zeros from the kept rows on, the static columns of kept row r against frame clamp(r skip - left + c), the refusals' codes.
#include <cstdio>
#include <cstdlib>

#include "../ctc_pytorch_amd/csrc/context.hip"

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
  const int ctx[4][2] = {{0, 0}, {0, 2}, {3, 3}, {5, 5}}, skips[5] = {0, 1, 2, 3, 7}, downs[3] = {1, 2, 4}, windows[3] = {1, 2, 5};
  long long calls = 0;
  for (int order = 0; order <= 2; ++order)
    for (int window : windows) {
      float *scales = static_cast<float *>(malloc(sizeof(float) * (2 * order * window + 1)));
      EXPECT(ctcn_delta_scales(order, window, scales) == 2 * order * window + 1);
      free(scales);
      for (int F : {1, 5})
        for (auto &lr : ctx)
          for (int skip : skips)
            for (int nd : downs) {
              ctcn_context_opts o = {lr[0], lr[1], skip, nd, order, window};
              EXPECT(ctcn_frame_context_tile(&o, F) >= 1);
              const int F1 = F * (order + 1), F2 = (lr[0] + 1 + lr[1]) * F1, s = skip > 1 ? skip : 1;
              for (int T = 0; T <= 40; ++T) {
                const int n_out = ctcn_context_frames(T, skip, nd), kept = (T + s - 1) / s;
                EXPECT(n_out >= kept && n_out % nd == 0 && n_out < kept + nd);
                float *x = static_cast<float *>(malloc(sizeof(float) * (size_t)T * F + 1));
                for (int i = 0; i < T * F; ++i) x[i] = (float)((i * 37) % 101) - 50.f;
                for (int extra : {0, 3}) {
                  const int rows = n_out + extra;
                  float *out = static_cast<float *>(malloc(sizeof(float) * (size_t)rows * F2 + 1));
                  float frac = -1.f;
                  EXPECT(ctcn_frame_context_host(x, T, F, &o, out, rows, &frac) == n_out);
                  ++calls;
                  EXPECT(frac == (rows ? (float)((double)n_out / (double)rows) : 0.f));
                  for (size_t i = (size_t)kept * F2; i < (size_t)rows * F2; ++i) EXPECT(out[i] == 0.f);
                  for (int r = 0; r < kept; ++r)
                    for (int c = 0; c < lr[0] + 1 + lr[1]; ++c) {
                      int u = r * s - lr[0] + c;
                      u = u < 0 ? 0 : (u > T - 1 ? T - 1 : u);
                      for (int f = 0; f < F; ++f) EXPECT(out[(size_t)r * F2 + (size_t)c * F1 + f] == x[(size_t)u * F + f]);
                    }
                  EXPECT(ctcn_frame_context_host(x, T, F, &o, out, n_out - 1, &frac) == CTCN_EINVAL);   // a buffer one row short
                  free(out);
                }
                free(x);
              }
            }
    }
  ctcn_context_opts bad = {0, 0, 1, 1, 3, 2};
  float one[8] = {0};
  EXPECT(ctcn_frame_context_tile(&bad, 1) == CTCN_EUNSUPPORTED && ctcn_frame_context_host(one, 1, 1, &bad, one, 1, nullptr) == CTCN_EUNSUPPORTED);
  EXPECT(ctcn_delta_scales(3, 2, one) == CTCN_EUNSUPPORTED && ctcn_delta_scales(1, 0, one) == CTCN_EINVAL);
  EXPECT(ctcn_context_frames(-1, 1, 1) == CTCN_EINVAL && ctcn_context_frames(0x7fffffff, 1, 1000) == CTCN_EUNSUPPORTED);
  printf("frame_context_host_check: %lld calls of ctcn_frame_context_host, no finding\n", calls);
  return 0;
}
