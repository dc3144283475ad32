// What the int4 weight-only kernels (skinny_gemm_w4.hip, moe_fused_w4.hip)
// share: the 128-wide quantization group, how many groups a loop iteration
// covers, and the in-register dequantizer. The packed layout is described in
// skinny_gemm_w4.hip.
#pragma once

#include "skinny_common.h"

typedef __attribute__((ext_vector_type(4))) unsigned int ps_w4u32x4;  // 16 B

#define PS_W4_GROUP 128
#define PS_W4_MAX_CPI 4  // most 128-wide groups per loop iteration

// groups per iteration of the M_TILES instantiation:
// (M_TILES, CPI) = (1, 4), (2, 2), (4, 2), (8, 1), (16, 1)
constexpr int ps_w4_cpi(int m_tiles) {
  return m_tiles == 1 ? 4 : m_tiles > 4 ? 1 : 2;
}

// eight nibbles of w -> (q - z) * s as eight bf16, element i from nibble i
PS_DEV ps_mfma_bf16x8 ps_w4_dequant8(unsigned int w, float s, float nzs) {
  const unsigned int lo = w & 0x0f0f0f0fu;         // elements 0, 2, 4, 6
  const unsigned int hi = (w >> 4) & 0x0f0f0f0fu;  // elements 1, 3, 5, 7
  union {
    ps_mfma_bf16x8 bf;
    unsigned int u[4];
  } o;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    ps_f32x2 p = {
        __builtin_fmaf((float)((lo >> (8 * b)) & 0xffu), s, nzs),
        __builtin_fmaf((float)((hi >> (8 * b)) & 0xffu), s, nzs)};
    ps_rawbf16x2 r = __builtin_convertvector(p, ps_rawbf16x2);
    o.u[b] = *(unsigned int*)&r;
  }
  return o.bf;
}
