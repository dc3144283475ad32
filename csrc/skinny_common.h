// What the split-K skinny GEMMs (skinny_gemm.hip, skinny_gemm_fp8.hip,
// skinny_gemm_w4.hip) share around their main loops: a workgroup's K-range,
// a lane's coordinates, the epilogue, the combine kernel and the M_TILES
// launch ladder. moe_fused.hip takes the operand type and the lane
// coordinates; gemm8p.hip the operand type and the combine kernel.
#pragma once

#include "ps_common.h"
#include "splitk.h"

// bf16 MFMA operand: the 16 bytes a lane loads as ps_bf16x8, retyped
typedef __attribute__((ext_vector_type(8))) __bf16 ps_mfma_bf16x8;

PS_DEV ps_mfma_bf16x8 ps_as_mfma_bf16(ps_bf16x8 u) {
  union {
    ps_bf16x8 u16;
    ps_mfma_bf16x8 bf;
  } v;
  v.u16 = u;
  return v.bf;
}

// K-units [begin, end) of split `split` out of `splits`; empty past the last
// non-empty split (ps_splitk_depth launches none of those).
struct ps_split_range {
  int begin, end;
};

PS_DEV ps_split_range ps_split_range_of(int units, int splits, int split) {
  const int per_split = (units + splits - 1) / splits;
  const int begin = split * per_split;
  return {begin, min(units, begin + per_split)};
}

// 256 threads = 4 waves x 16 W rows; the lane is row/col rc of its 16x16
// tiles and k-group g. nrow is the lane's W row, i.e. its B and C column.
struct ps_skinny_lane {
  int wave, g, rc, nrow;
};

PS_DEV ps_skinny_lane ps_skinny_lane_of() {
  const int n0 = blockIdx.x * 64;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int g = lane >> 4;
  const int rc = lane & 15;
  return {wave, g, rc, n0 + wave * 16 + rc};
}

// Epilogue (C layout: row = g*4 + r, col = rc of each 16x16 tile). A lone
// split writes the bf16 output directly; otherwise each split streams its
// unscaled fp32 partial to ws[split][M][N] and a combine kernel reduces:
// device atomicAdd RMW traffic (M*N*splits) was the measured 1/M throughput
// wall of the earlier design.
// SCALED is the value rounded to bf16, written in terms of the sum `v` and
// its row `m`; the macro reads the kernel's out_bf16, ws, acc, M, N, g, nrow.
// A macro because, as an inlined function over a scale functor, hipcc emits
// other code for it than for the loop written out in the kernel: it reloads
// the grid size per element, or at best swaps multiplicand operands.
#define PS_SKINNY_EPILOGUE(SCALED)                                 \
  _Pragma("unroll") for (int mt = 0; mt < M_TILES; mt++) {         \
    _Pragma("unroll") for (int r = 0; r < 4; r++) {                \
      const int m = mt * 16 + g * 4 + r;                           \
      if (m >= M) continue;                                        \
      const float v = acc[mt][r];                                  \
      if (gridDim.y == 1) {                                        \
        out_bf16[(long)m * N + nrow] = ps_f32_to_bf16(SCALED);     \
      } else {                                                     \
        ws[((long)blockIdx.y * M + m) * N + nrow] = v;             \
      }                                                            \
    }                                                              \
  }

// out[M, N] bf16 = scale(sum over splits of ws[S, M, N], flat index), summed
// in split order by one thread per output.
template <class Scale>
PS_DEV void ps_splitk_combine(unsigned short* out, const float* ws, long MN,
                              int splits, Scale scale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN) return;
  float acc = 0.f;
  for (int s = 0; s < splits; s++) acc += ws[(long)s * MN + i];
  out[i] = ps_f32_to_bf16(scale(acc, i));
}

struct ps_no_scale {
  PS_DEV float operator()(float acc, long) const { return acc; }
};

// The combine as a kernel. bf16, w4 and gemm8p launch the ps_no_scale one;
// the fp8 GEMM keeps a kernel of its own around ps_splitk_combine, whose
// arguments stay in the order they had. static: a file that launches it has
// its own copy, like every other kernel of that file.
template <class Scale>
static __global__ __launch_bounds__(256) void ps_splitk_combine_kernel(
    unsigned short* __restrict__ out,  // [M, N] bf16
    const float* __restrict__ ws,      // [S, M, N] fp32
    long MN, int splits, Scale scale) {
  ps_splitk_combine(out, ws, MN, splits, scale);
}

template <class Scale = ps_no_scale>
void ps_launch_splitk_combine(void* out_bf16, const void* ws, int M, int N,
                              int splits, hipStream_t stream,
                              Scale scale = Scale()) {
  const long MN = (long)M * N;
  ps_splitk_combine_kernel<<<dim3((MN + 255) / 256), 256, 0, stream>>>(
      (unsigned short*)out_bf16, (const float*)ws, MN, splits, scale);
}

// LAUNCH(M_TILES) for the smallest instantiation that holds M <= 256 rows
#define PS_SKINNY_M_LADDER(M, LAUNCH) \
  do {                                \
    if ((M) <= 16) LAUNCH(1);         \
    else if ((M) <= 32) LAUNCH(2);    \
    else if ((M) <= 64) LAUNCH(4);    \
    else if ((M) <= 128) LAUNCH(8);   \
    else LAUNCH(16);                  \
  } while (0)
