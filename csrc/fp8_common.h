// What the fp8 GEMMs (skinny_gemm_fp8.hip, gemm_fp8_tiled.hip) share: the
// scale applied once to a full fp32 sum, and the split-K combine around it.
#pragma once

#include "skinny_common.h"

// out = acc * (sx[m] * sw[n]): the scale product is formed first, in fp32
struct ps_f8_scale {
  const float* sx;  // [M]
  const float* sw;  // [N]
  int N;
  PS_DEV float operator()(float acc, long i) const {
    return acc * (sx[i / N] * sw[i % N]);
  }
};

// static: a file that launches it has its own copy, like every other kernel
// of that file.
static __global__ __launch_bounds__(256) void skinny_fp8_combine_kernel(
    unsigned short* __restrict__ out,  // [M, N] bf16
    const float* __restrict__ ws,      // [S, M, N] fp32, unscaled
    const float* __restrict__ sx, const float* __restrict__ sw, long MN,
    int N, int splits) {
  ps_splitk_combine(out, ws, MN, splits, ps_f8_scale{sx, sw, N});
}

static inline void ps_launch_fp8_combine(void* out_bf16, const void* ws,
                                         const void* sx, const void* sw,
                                         int M, int N, int splits,
                                         hipStream_t stream) {
  const long MN = (long)M * N;
  skinny_fp8_combine_kernel<<<dim3((MN + 255) / 256), 256, 0, stream>>>(
      (unsigned short*)out_bf16, (const float*)ws, (const float*)sx,
      (const float*)sw, MN, N, splits);
}
