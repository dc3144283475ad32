// fp8 skinny-batch GEMM for decode steps:
//   out[M, N] bf16 = (xq[M, K] * sx[M, None]) @ (wq[N, K] * sw[N, None])^T
// xq / wq OCP e4m3, sx / sw fp32, fp32 accumulation, 1 <= M <= 256.
//
// Same plan as skinny_gemm.hip (the op is weight-bandwidth-bound, so W is
// streamed exactly once and everything else is arranged around that) with
// half the bytes per weight:
//   grid = (N/64, SPLITS): a workgroup owns 64 N-rows x a K-range counted in
//   64-wide chunks. 4 waves x 16 N-rows; each lane reads its own W row with
//   one 16-B load per chunk.
//   A 64-wide fp8 chunk is only 64 B per row, half of the bf16 kernel's, so
//   an iteration covers up to PS_F8_CPI chunks: the W loads of all of them
//   are issued first (64 B per lane in flight), then the x chunks are staged
//   in LDS, then the MFMAs run chunk by chunk in ascending k.
//   mfma_f32_16x16x32_fp8_fp8 takes 8 fp8 per lane per operand. Lane (g, rc)
//   feeds bytes [16g, 16g+8) of its A row and of its B row to the first MFMA
//   of a chunk and bytes [16g+8, 16g+16) to the second. A and B use the same
//   k offsets, so whatever order the instruction gives the 32 k inside it,
//   the sum pairs x[m][k] with w[n][k]; only the row/col lane map (lane&15)
//   and the C/D map (col = lane&15, row = 4*(lane>>4) + r, as for bf16)
//   matter.
//   Split-K partials go unscaled to ws[SPLITS, M, N] fp32 and a combine
//   kernel sums them in split order; sx[m]*sw[n] is applied once in fp32
//   right before the bf16 round (GEMM epilogue when SPLITS == 1, combine
//   kernel otherwise). No atomics: results are bit-deterministic.
//   A row's result does not depend on M: SPLITS is a function of (N, K), and
//   every M_TILES instantiation accumulates chunk by chunk in the same order.
//
// LDS image: one [MP][64 B] sub-image per chunk, 4 16-B slots per row, so
// four rows share a 256-B bank row. ds_read_b128 is served in 16-lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32 for the upper half): a group
// holds rows with q = (row>>2)&3 in {0,3} at slot g and q in {1,2} at slot
// g^1, for every row&3. Storing slot s of a row at s ^ f(q) with
// f = {0,2,3,1} gives the four (g, q) pairs of a group four different slots,
// so the 16 lanes cover the 16 slots of the bank row: conflict-free. (The
// plain s ^ q leaves q=0/q=1 and q=3/q=2 on one slot: 2-way.) The staging
// ds_write_b128 goes in groups of 8 consecutive lanes = 2 rows x 4 slots =
// one 128-B span, conflict-free under its 32-bank rule with or without the
// XOR.
//
// The K-range, lane coordinates, epilogue, combine loop and launch ladder are
// csrc/skinny_common.h's; the split depth is csrc/splitk.h's.
#include "skinny_common.h"

typedef __attribute__((ext_vector_type(2))) long ps_f8x16;  // 16 fp8, 16 B

#define PS_F8_CPI 4  // 64-wide k-chunks per loop iteration

PS_DEV int ps_f8_swz(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }

template <int M_TILES>
__global__ __launch_bounds__(256) void skinny_gemm_fp8_kernel(
    unsigned short* __restrict__ out_bf16,  // [M, N] (splits == 1)
    float* __restrict__ ws,                 // [S, M, N] (splits > 1)
    const unsigned char* __restrict__ xq,   // [M, K] e4m3
    const float* __restrict__ sx,           // [M]
    const unsigned char* __restrict__ wq,   // [N, K] e4m3
    const float* __restrict__ sw,           // [N]
    int M, int N, int K) {
  constexpr int MP = M_TILES * 16;  // padded M
  const auto [kc_begin, kc_end] =
      ps_split_range_of(K / 64, gridDim.y, blockIdx.y);
  if (kc_begin >= kc_end) return;

  const int tid = threadIdx.x;
  const auto [wave, g, rc, nrow] = ps_skinny_lane_of();

  __shared__ __align__(16) unsigned char x_lds[PS_F8_CPI][MP][64];

  ps_f32x4 acc[M_TILES];
#pragma unroll
  for (int mt = 0; mt < M_TILES; mt++) acc[mt] = {0.f, 0.f, 0.f, 0.f};

  const unsigned char* wrow = wq + (long)nrow * K + g * 16;

  for (int kc = kc_begin; kc < kc_end; kc += PS_F8_CPI) {
    const int nc = min(PS_F8_CPI, kc_end - kc);  // chunks this iteration
    // ---- B-frags first: W rows streamed once, up to 64 B per lane ----
    ps_f8x16 b[PS_F8_CPI];
#pragma unroll
    for (int c = 0; c < PS_F8_CPI; c++) {
      b[c] = {0, 0};
      if (c < nc) b[c] = *(const ps_f8x16*)(wrow + (long)(kc + c) * 64);
    }
    // ---- cooperative x staging: nc*MP*4 16-B slots over 256 threads ----
    for (int u = tid; u < nc * MP * 4; u += 256) {
      const int c = u / (MP * 4);
      const int row = (u >> 2) & (MP - 1);
      const int slot = u & 3;
      ps_f8x16 v = {0, 0};
      if (row < M)
        v = *(const ps_f8x16*)(xq + (long)row * K + (long)(kc + c) * 64 +
                               slot * 16);
      *(ps_f8x16*)(&x_lds[c][row][(slot ^ ps_f8_swz(row)) * 16]) = v;
    }
    __syncthreads();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < PS_F8_CPI; c++) {
      if (c < nc) {
#pragma unroll
        for (int mt = 0; mt < M_TILES; mt++) {
          const int row = mt * 16 + rc;
          const ps_f8x16 a =
              *(const ps_f8x16*)(&x_lds[c][row][(g ^ ps_f8_swz(row)) * 16]);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              a[0], b[c][0], acc[mt], 0, 0, 0);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              a[1], b[c][1], acc[mt], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }

  // sx[m] * sw[n] is formed first, in fp32, and applied once to the full sum
  const float swn = sw[nrow];
  PS_SKINNY_EPILOGUE(v * (sx[m] * swn));
}

struct ps_f8_scale {
  const float* sx;  // [M]
  const float* sw;  // [N]
  int N;
  PS_DEV float operator()(float acc, long i) const {
    return acc * (sx[i / N] * sw[i % N]);
  }
};

__global__ __launch_bounds__(256) void skinny_fp8_combine_kernel(
    unsigned short* __restrict__ out,  // [M, N] bf16
    const float* __restrict__ ws,      // [S, M, N] fp32, unscaled
    const float* __restrict__ sx, const float* __restrict__ sw, long MN,
    int N, int splits) {
  ps_splitk_combine(out, ws, MN, splits, ps_f8_scale{sx, sw, N});
}

extern "C" {

// Split depth for a shape, a function of (N, K) only; -1 if unsupported.
// A split's chunk count is rounded up to whole PS_F8_CPI iterations.
int ps_skinny_gemm_fp8_splits(int M, int N, int K) {
  if (M < 1 || M > 256 || N < 64 || K < 64 || N % 64 != 0 || K % 64 != 0)
    return -1;
  return ps_splitk_depth(K / 64, N / 64, 1024, PS_F8_CPI);
}

// ws == nullptr forces splits = 1.
int ps_skinny_gemm_fp8(void* out_bf16, void* ws, const void* xq,
                       const void* sx, const void* wq, const void* sw, int M,
                       int N, int K, hipStream_t stream) {
  int splits = ps_skinny_gemm_fp8_splits(M, N, K);
  if (splits < 0) return -1;
  if (ws == nullptr) splits = 1;
  dim3 grid(N / 64, splits);
  dim3 block(256);
#define PS_SGF(MT)                                                         \
  skinny_gemm_fp8_kernel<MT><<<grid, block, 0, stream>>>(                  \
      (unsigned short*)out_bf16, (float*)ws, (const unsigned char*)xq,     \
      (const float*)sx, (const unsigned char*)wq, (const float*)sw, M, N, K)
  PS_SKINNY_M_LADDER(M, PS_SGF);
#undef PS_SGF
  if (splits > 1) {
    const long MN = (long)M * N;
    skinny_fp8_combine_kernel<<<dim3((MN + 255) / 256), 256, 0, stream>>>(
        (unsigned short*)out_bf16, (const float*)ws, (const float*)sx,
        (const float*)sw, MN, N, splits);
  }
  return 0;
}

}  // extern "C"
