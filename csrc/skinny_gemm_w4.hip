// int4 weight-only (W4A16) skinny-batch GEMM for decode steps, and the
// dequantizer that serves everything the GEMM does not take:
//   out[M, N] bf16 = x[M, K] bf16 @ W_deq[N, K]^T, 1 <= M <= 256
//   W_deq[n, k] = bf16_rne(float(q[n, k] - z[n, k/128]) * float(s[n, k/128]))
// q in 0..15, z uint8 in 0..15, s bf16, one (s, z) per 128 k of a row. The
// MFMA operands are exactly these bf16 values and accumulation is fp32, so
// the result is x @ W_deq^T of the dequantized matrix, not a rescaled sum.
//
// Packed layout (ops.int4_pack / ops.int4_unpack are the only other places
// that know it). A row of `packed` is K/2 bytes, a 128-wide k-group is 64 B:
//   k = 128*c + 32*j + 8*g + i   (c group, j in 0..3, g in 0..3, i in 0..7)
//   lives in nibble i of the little-endian dword at byte 64*c + 16*g + 4*j,
//   i.e. byte 64*c + 16*g + 4*j + i/2, low nibble for even i.
// One 16-B lane load at 64*c + 16*g therefore yields dwords j = 0..3, and
// dword j holds the eight k (32*j + 8*g ..+7) that lane g feeds to MFMA j of
// the group: the same k-runs the bf16 kernel reads from W, with no
// cross-lane move. Within a dword, `w & 0x0f0f0f0f` leaves the even nibbles
// one per byte and `(w >> 4) & 0x0f0f0f0f` the odd ones, so each element
// costs one v_cvt_f32_ubyteN, one fma and half a v_cvt_pk_bf16_f32:
//   fma(float(q), s, -(float(z) * s)) = (q - z) * s exactly (5-bit integer
//   times 8-bit significand; both products are exact and the fma rounds
//   once), and the fp32 -> bf16 convert is round-to-nearest-even.
//
// GEMM plan, as skinny_gemm.hip / skinny_gemm_fp8.hip (the op is
// weight-bandwidth-bound; W is streamed exactly once):
//   grid = (N/64, SPLITS): a workgroup owns 64 N-rows x a K-range counted in
//   128-wide groups. 4 waves x 16 N-rows; each lane reads its own W row.
//   A group is only 64 B per row, so an iteration covers up to CPI groups:
//   all their W loads are issued first, then the x chunks are staged in LDS,
//   then each group is dequantized in registers and its 4 MFMAs per m-tile
//   run, groups in ascending k. CPI shrinks as M_TILES grows to bound LDS
//   (CPI * MP * 256 B <= 64 KiB); the accumulation order does not change
//   with it.
//   Split-K partials go to ws[SPLITS, M, N] fp32 and a combine kernel sums
//   them in split order. No atomics: results are bit-deterministic.
//   A row's result does not depend on M: SPLITS is a function of (N, K), and
//   every M_TILES instantiation accumulates group by group in the same
//   order.
//
// LDS image: [MP][128] bf16 per group, 16 16-B slots per 256-B row; slot t
// of a row is stored at t ^ (row & 15). A ds_read_b128 is served in 16-lane
// groups that hold 8 rows at slot 4j+g and 8 other rows at slot 4j+(g^1);
// the XOR sends those 16 (row, slot) pairs to 16 different slots of the
// 256-B bank row.
//
// The K-range, lane coordinates, epilogue, combine kernel and launch ladder
// are csrc/skinny_common.h's; the split depth is csrc/splitk.h's.
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

template <int M_TILES, int CPI>
__global__ __launch_bounds__(256) void skinny_gemm_w4_kernel(
    unsigned short* __restrict__ out_bf16,    // [M, N] (splits == 1)
    float* __restrict__ ws,                   // [S, M, N] (splits > 1)
    const unsigned short* __restrict__ x,     // [M, K] bf16
    const unsigned char* __restrict__ wp,     // [N, K/2] packed nibbles
    const unsigned short* __restrict__ sc,    // [N, K/128] bf16
    const unsigned char* __restrict__ zp,     // [N, K/128]
    int M, int N, int K) {
  constexpr int MP = M_TILES * 16;  // padded M
  const int kgroups = K / PS_W4_GROUP;
  const auto [kc_begin, kc_end] =
      ps_split_range_of(kgroups, gridDim.y, blockIdx.y);
  if (kc_begin >= kc_end) return;

  const int tid = threadIdx.x;
  const auto [wave, g, rc, nrow] = ps_skinny_lane_of();

  __shared__ __align__(16) unsigned short x_lds[CPI][MP][PS_W4_GROUP];

  ps_f32x4 acc[M_TILES];
#pragma unroll
  for (int mt = 0; mt < M_TILES; mt++) acc[mt] = {0.f, 0.f, 0.f, 0.f};

  const unsigned char* wrow = wp + (long)nrow * (K / 2) + g * 16;
  const unsigned short* srow = sc + (long)nrow * kgroups;
  const unsigned char* zrow = zp + (long)nrow * kgroups;

  for (int kc = kc_begin; kc < kc_end; kc += CPI) {
    const int nc = min(CPI, kc_end - kc);  // groups this iteration
    // ---- packed W first: rows streamed once, up to 64 B per lane ----
    ps_w4u32x4 b[CPI];
    float s[CPI], nzs[CPI];
#pragma unroll
    for (int c = 0; c < CPI; c++) {
      b[c] = {0u, 0u, 0u, 0u};
      s[c] = 0.f;
      nzs[c] = 0.f;
      if (c < nc) {
        b[c] = *(const ps_w4u32x4*)(wrow + (long)(kc + c) * 64);
        s[c] = ps_bf16_to_f32(srow[kc + c]);
        nzs[c] = -((float)zrow[kc + c] * s[c]);
      }
    }
    // ---- cooperative x staging: nc*MP*16 16-B slots over 256 threads ----
    for (int u = tid; u < nc * MP * 16; u += 256) {
      const int c = u / (MP * 16);
      const int row = (u >> 4) & (MP - 1);
      const int slot = u & 15;
      ps_bf16x8 v = {};
      if (row < M)
        v = *(const ps_bf16x8*)(x + (long)row * K +
                                (long)(kc + c) * PS_W4_GROUP + slot * 8);
      *(ps_bf16x8*)(&x_lds[c][row][(slot ^ (row & 15)) * 8]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CPI; c++) {
      if (c < nc) {
        // ---- B-frags built in registers ----
        ps_mfma_bf16x8 bf[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
          bf[j] = ps_w4_dequant8(b[c][j], s[c], nzs[c]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int mt = 0; mt < M_TILES; mt++) {
          const int row = mt * 16 + rc;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const ps_mfma_bf16x8 a = *(const ps_mfma_bf16x8*)(
                &x_lds[c][row][((4 * j + g) ^ (row & 15)) * 8]);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, bf[j], acc[mt], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __syncthreads();
  }

  PS_SKINNY_EPILOGUE(v);
}

// packed + s + z -> W_deq[N, K] bf16. One thread per 16-B packed load (32
// elements): four 16-B stores, and the four threads of a group's g = 0..3
// cover 64 contiguous bytes per store.
__global__ __launch_bounds__(256) void int4_dequant_kernel(
    unsigned short* __restrict__ out,       // [N, K] bf16
    const unsigned char* __restrict__ wp,   // [N, K/2]
    const unsigned short* __restrict__ sc,  // [N, K/128]
    const unsigned char* __restrict__ zp,   // [N, K/128]
    long total /* N * K/128 * 4 */, int K) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int g = (int)(t & 3);
  const long ng = t >> 2;  // n * kgroups + c
  const int kgroups = K / PS_W4_GROUP;
  const long n = ng / kgroups;
  const int c = (int)(ng - n * kgroups);
  const ps_w4u32x4 w = *(const ps_w4u32x4*)(wp + t * 16);
  const float s = ps_bf16_to_f32(sc[ng]);
  const float nzs = -((float)zp[ng] * s);
  unsigned short* o = out + n * K + (long)c * PS_W4_GROUP + g * 8;
#pragma unroll
  for (int j = 0; j < 4; j++)
    *(ps_mfma_bf16x8*)(o + 32 * j) = ps_w4_dequant8(w[j], s, nzs);
}

extern "C" {

// Split depth for a shape, a function of (N, K) only; -1 if unsupported.
// A split's group count is rounded up to whole PS_W4_MAX_CPI iterations.
int ps_skinny_gemm_w4_splits(int M, int N, int K) {
  if (M < 1 || M > 256 || N < 64 || K < PS_W4_GROUP || N % 64 != 0 ||
      K % PS_W4_GROUP != 0)
    return -1;
  return ps_splitk_depth(K / PS_W4_GROUP, N / 64, 1024, PS_W4_MAX_CPI);
}

// ws == nullptr forces splits = 1.
int ps_skinny_gemm_w4(void* out_bf16, void* ws, const void* x,
                      const void* packed, const void* scales,
                      const void* zeros, int M, int N, int K,
                      hipStream_t stream) {
  int splits = ps_skinny_gemm_w4_splits(M, N, K);
  if (splits < 0) return -1;
  if (ws == nullptr) splits = 1;
  dim3 grid(N / 64, splits);
  dim3 block(256);
#define PS_SGW(MT)                                                          \
  skinny_gemm_w4_kernel<MT, ps_w4_cpi(MT)><<<grid, block, 0, stream>>>(     \
      (unsigned short*)out_bf16, (float*)ws, (const unsigned short*)x,      \
      (const unsigned char*)packed, (const unsigned short*)scales,          \
      (const unsigned char*)zeros, M, N, K)
  PS_SKINNY_M_LADDER(M, PS_SGW);
#undef PS_SGW
  if (splits > 1)
    ps_launch_splitk_combine(out_bf16, ws, M, N, splits, stream);
  return 0;
}

// Any N >= 1; K a multiple of the group size.
int ps_int4_dequant(void* out_bf16, const void* packed, const void* scales,
                    const void* zeros, long N, int K, hipStream_t stream) {
  if (N < 1 || K < PS_W4_GROUP || K % PS_W4_GROUP != 0) return -1;
  const long total = N * (K / PS_W4_GROUP) * 4;
  int4_dequant_kernel<<<dim3((total + 255) / 256), 256, 0, stream>>>(
      (unsigned short*)out_bf16, (const unsigned char*)packed,
      (const unsigned short*)scales, (const unsigned char*)zeros, total, K);
  return 0;
}

}  // extern "C"
