// A/B of gemm_fp8_tiled's two MFMA forms at one shape: the gfx950 128-deep
// v_mfma_f32_16x16x128_f8f6f4 against four mfma_f32_16x16x32_fp8_fp8 on the
// same registers. Everything else of the kernel (tiling, LDS images, pipeline,
// epilogue) is shared, so the difference is the instruction's.
// Both forms run on the same seeded operands; the outputs are compared first,
// then timed in alternating windows between hip events: median us of ROUNDS
// windows of CALLS calls with the min..max spread, and 2*M*N*K / median.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 gemm_fp8_tiled_ab.hip \
//            -o gemm_fp8_tiled_ab
// Run:   gemm_fp8_tiled_ab [M N K]      (default 4096 28672 4096)
#include "../gemm_fp8_tiled.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                      \
  do {                                                                \
    hipError_t e_ = (x);                                              \
    if (e_ != hipSuccess) {                                           \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static const int ROUNDS = 7;
static const int CALLS = 40;

int main(int argc, char** argv) {
  const int M = argc > 3 ? atoi(argv[1]) : 4096;
  const int N = argc > 3 ? atoi(argv[2]) : 28672;
  const int K = argc > 3 ? atoi(argv[3]) : 4096;
  if (ps_f8t_splits(M, N, K) < 0) {
    fprintf(stderr, "unsupported shape %d %d %d\n", M, N, K);
    return 1;
  }
  // finite e4m3 codes only: magnitude bits < 0x78
  std::vector<unsigned char> hx((size_t)M * K), hw((size_t)N * K);
  unsigned s = 12345u;
  auto code = [&]() {
    s = s * 1664525u + 1013904223u;
    const unsigned v = s >> 16;
    return (unsigned char)((v % 0x78u) | ((v >> 8) & 1u) << 7);
  };
  for (auto& b : hx) b = code();
  for (auto& b : hw) b = code();
  std::vector<float> hsx(M, 1.f / 512), hsw(N, 1.f / 512);

  unsigned char *xq, *wq;
  float *sx, *sw;
  unsigned short* out[2];
  CHECK(hipMalloc(&xq, hx.size()));
  CHECK(hipMalloc(&wq, hw.size()));
  CHECK(hipMalloc(&sx, M * sizeof(float)));
  CHECK(hipMalloc(&sw, N * sizeof(float)));
  for (auto& o : out) CHECK(hipMalloc(&o, (size_t)M * N * 2));
  CHECK(hipMemcpy(xq, hx.data(), hx.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(wq, hw.data(), hw.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(sx, hsx.data(), M * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(sw, hsw.data(), N * sizeof(float), hipMemcpyHostToDevice));

  // one split for both forms: the A/B is of the main loop
  auto run = [&](int deep) {
    return deep ? ps_f8t_launch<true>(out[1], nullptr, xq, sx, wq, sw, M, N,
                                      K, 0)
                : ps_f8t_launch<false>(out[0], nullptr, xq, sx, wq, sw, M, N,
                                       K, 0);
  };
  for (int w = 0; w < 3; w++)
    for (int deep = 0; deep < 2; deep++)
      if (run(deep) != 0) return 1;
  CHECK(hipDeviceSynchronize());

  std::vector<unsigned short> h0((size_t)M * N), h1((size_t)M * N);
  CHECK(hipMemcpy(h0.data(), out[0], h0.size() * 2, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(h1.data(), out[1], h1.size() * 2, hipMemcpyDeviceToHost));
  size_t differ = 0, far = 0;
  for (size_t i = 0; i < h0.size(); i++) {
    if (h0[i] == h1[i]) continue;
    differ++;
    // more than one bf16 step apart (same sign) or a sign flip
    const int d = (int)h0[i] - (int)h1[i];
    if (d > 1 || d < -1) far++;
  }
  printf("AB shape %d %d %d: %zu/%zu outputs differ, %zu by more than one "
         "bf16 step\n", M, N, K, differ, h0.size(), far);

  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  std::vector<float> us[2];
  for (int r = 0; r < ROUNDS; r++)
    for (int deep = 0; deep < 2; deep++) {
      CHECK(hipEventRecord(t0, 0));
      for (int c = 0; c < CALLS; c++) run(deep);
      CHECK(hipEventRecord(t1, 0));
      CHECK(hipEventSynchronize(t1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, t0, t1));
      us[deep].push_back(ms * 1e3f / CALLS);
    }
  for (int deep = 0; deep < 2; deep++) {
    std::sort(us[deep].begin(), us[deep].end());
    const float med = us[deep][ROUNDS / 2];
    printf("AB %s: %.1f us (%.1f..%.1f), %.1f TFLOP/s\n",
           deep ? "16x16x128_f8f6f4" : "4 x 16x16x32_fp8_fp8", med,
           us[deep].front(), us[deep].back(),
           2.0 * M * N * K / med / 1e6);
  }
  return 0;
}
