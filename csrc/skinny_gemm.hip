// Skinny-batch GEMM for decode steps: out[M, N] = x[M, K] @ W[N, K]^T,
// bf16 inputs, fp32 accumulation, M <= 256.
//
// Why it exists: hipBLASLt's tile selection for the decode-shaped GEMMs
// (qkv [M,4096]x[6144,4096], o, down) streams weights at only 1.4-2 TB/s at
// M in 16..128 (profiles/gemm_plain.log) when the op is purely
// weight-bandwidth-bound (~6 TB/s available). This kernel is built around
// streaming W exactly once:
//   grid = (N/64, SPLITS): workgroup owns 64 N-rows x a K-range.
//   4 waves x 16 N-rows each; B-frags are direct 16-B lane loads from W
//   (lane's col = its N-row, contiguous dims) -- W bytes are read once
//   across the whole grid.
//   x (tiny) is staged per 64-wide K-chunk in XOR-swizzled LDS and consumed
//   as A-frags for ceil(M/16) m-tiles; per-k-chunk MFMA count scales with
//   m-tiles while W traffic stays fixed.
//   Split-K partials go to an fp32 workspace ws[SPLITS, M, N] and a combine
//   kernel sums them to bf16 (no atomics; every split writes its slice).
// mfma_f32_16x16x32_bf16; operand k-pattern as verified in
// csrc/tools/mfma_probe.hip.
// The K-range, lane coordinates, epilogue, combine kernel and launch ladder
// are csrc/skinny_common.h's; the split depth is csrc/splitk.h's.
#include "skinny_common.h"

template <int M_TILES>
__global__ __launch_bounds__(256, 4) void skinny_gemm_kernel(
    unsigned short* __restrict__ out_bf16,  // [M, N] (splits == 1)
    float* __restrict__ ws,                 // [S, M, N] (splits > 1)
    const unsigned short* __restrict__ x,   // [M, K]
    const unsigned short* __restrict__ w,   // [N, K]
    int M, int N, int K, long x_stride /* row stride of x, elems */) {
  constexpr int MP = M_TILES * 16;  // padded M
  const auto [kc_begin, kc_end] =
      ps_split_range_of(K / 64, gridDim.y, blockIdx.y);
  if (kc_begin >= kc_end) return;

  const int tid = threadIdx.x;
  const auto [wave, g, rc, nrow] = ps_skinny_lane_of();

  // x chunk [MP][64] staged with 16-B slot XOR swizzle (slot ^= row&7)
  __shared__ __align__(16) unsigned short x_lds[MP][64];

  ps_f32x4 acc[M_TILES];
#pragma unroll
  for (int mt = 0; mt < M_TILES; mt++) acc[mt] = {0.f, 0.f, 0.f, 0.f};

  for (int kc = kc_begin; kc < kc_end; kc++) {
    // ---- cooperative x staging: MP*8 16-B slots over 256 threads ----
    for (int u = tid; u < MP * 8; u += 256) {
      const int row = u >> 3;
      const int slot = u & 7;
      ps_bf16x8 v = {};
      if (row < M)
        v = *(const ps_bf16x8*)(x + (long)row * x_stride + kc * 64 +
                                slot * 8);
      *(ps_bf16x8*)(&x_lds[row][(slot ^ (row & 7)) * 8]) = v;
    }
    __syncthreads();
    // ---- B-frags: W rows streamed once ----
    const unsigned short* wr = w + (long)nrow * K + kc * 64;
    ps_mfma_bf16x8 b0 = ps_as_mfma_bf16(*(const ps_bf16x8*)(wr + g * 8));
    ps_mfma_bf16x8 b1 =
        ps_as_mfma_bf16(*(const ps_bf16x8*)(wr + 32 + g * 8));
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mt = 0; mt < M_TILES; mt++) {
      const int row = mt * 16 + rc;
      ps_mfma_bf16x8 a0 = ps_as_mfma_bf16(
          *(const ps_bf16x8*)(&x_lds[row][(g ^ (row & 7)) * 8]));
      ps_mfma_bf16x8 a1 = ps_as_mfma_bf16(
          *(const ps_bf16x8*)(&x_lds[row][((4 + g) ^ (row & 7)) * 8]));
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[mt],
                                                        0, 0, 0);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[mt],
                                                        0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }

  PS_SKINNY_EPILOGUE(v);
}

extern "C" {

// ws == nullptr forces splits = 1. ps_skinny_gemm_splits reports the
// split depth the heuristic will pick for a shape so the caller can size
// the fp32 workspace.
int ps_skinny_gemm_splits(int M, int N, int K) {
  if (M < 1 || M > 256 || N < 64 || K < 64 || N % 64 != 0 || K % 64 != 0)
    return -1;
  return ps_splitk_depth(K / 64, N / 64, 1024, 1);
}

int ps_skinny_gemm(void* out_bf16, void* ws, const void* x, const void* w,
                   int M, int N, int K, long x_stride, hipStream_t stream) {
  int splits = ps_skinny_gemm_splits(M, N, K);
  if (splits < 0) return -1;
  if (ws == nullptr) splits = 1;
  dim3 grid(N / 64, splits);
  dim3 block(256);
#define PS_SG(MT)                                                           \
  skinny_gemm_kernel<MT><<<grid, block, 0, stream>>>(                       \
      (unsigned short*)out_bf16, (float*)ws, (const unsigned short*)x,      \
      (const unsigned short*)w, M, N, K, x_stride)
  PS_SKINNY_M_LADDER(M, PS_SG);
#undef PS_SG
  if (splits > 1)
    ps_launch_splitk_combine(out_bf16, ws, M, N, splits, stream);
  return 0;
}

}  // extern "C"
