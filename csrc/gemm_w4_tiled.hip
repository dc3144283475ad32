// int4 weight-only (W4A16) GEMM tiled in M and N, for prefill-sized steps:
//   out[M, N] bf16 = x[M, K] bf16 @ W_deq[N, K]^T, M >= 1
// Format, packed layout and numerics are skinny_gemm_w4.hip's: the MFMA
// operands are exactly the bf16 values ps_w4_dequant8 produces, accumulation
// is fp32. skinny_gemm_w4 streams W once and re-reads x from LDS for every
// MFMA, which is right while W dominates the traffic (M <= 256); here a
// workgroup dequantizes a W tile once into LDS and both operands are reused
// from registers.
//
// Plan:
//   Tile 128 (M) x 128 (N) per workgroup, 256 threads, waves 2 x 2, each
//   owning 64 x 64 = 4 x 4 tiles of mfma_f32_16x16x32_bf16 (64 accumulator
//   VGPRs). Per 32-wide k-step a wave reads 4 A-frags and 4 B-frags and
//   issues 16 MFMAs: 2 MFMAs per ds_read_b128.
//   K step = one 128-wide quantization group:
//     W: 128 rows x 64 B packed, two 16-B loads per thread (row t/4 and
//        t/4 + 64, lane group g = t%4) plus that row's s and z. The thread
//        dequantizes its 2 x 32 elements and writes them as bf16 to the B
//        image [128][128]: dword j of the load is k-slot 4j + g of the row
//        (see the layout note in skinny_gemm_w4.hip).
//     x: 128 rows x 256 B, eight 16-B loads per thread (slot t%16, rows
//        t/16 + 16i), to the A image [128][128].
//   Both images use x_lds's swizzle of skinny_gemm_w4.hip: slot t of a row is
//   stored at t ^ (row & 15), which makes the frag reads (16 rows at slot
//   4j+g per 16-lane group) conflict-free.
//   LDS is single-buffered, 2 x 32 KiB = 64 KiB, so two workgroups fit a
//   CU's 160 KiB and one's staging is covered by the other's MFMAs. Within a
//   workgroup the global loads of group c+1 are issued into registers before
//   the MFMAs of group c and are dequantized and written to LDS after them;
//   two barriers per group (reads done before the overwrite, writes done
//   before the reads).
//   Tails: an x row >= M, or a W row >= N of the 64-row last tile that
//   N % 128 == 64 leaves, reads the last valid row in its place and is never
//   stored (zero-filling them compiled to one exec-mask branch per load, ten
//   per group). Waves whose 64 x 64 block lies wholly past an edge skip their
//   MFMAs.
//   Grid = (tiles rounded up to 8, splits); tiles are numbered M-fastest
//   behind gemm8p's bijective XCD remap, so the workgroups that are
//   consecutive on one XCD share an N tile's weights in its L2.
//   Split-K over whole groups for launches that would leave CUs idle: fp32
//   partials to ws[S, M, N], summed in split order by the shared combine
//   kernel. No atomics: bit-deterministic for a fixed (M, N, K). The depth
//   depends on the tile count, so unlike skinny_gemm_w4 a row's bits may
//   depend on M.
#include "w4_common.h"

// No packed-fp32 VALU ops (v_pk_fma_f32 and kin) in this file's device code:
// the dequantizer's fma pairs are emitted as scalar fmas instead.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                  \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define PS_W4T_BM 128
#define PS_W4T_BN 128

// Workgroups resident at once, the grid size split-K aims for: 256 CUs x 2
// workgroups per CU. Both limits give 2: LDS (64 KiB each of 160 KiB) and
// VGPRs (<= 256 per lane, so 2 waves per SIMD, one per workgroup).
#define PS_W4T_TARGET_WGS 512

__global__ __launch_bounds__(256, 2) void gemm_w4_tiled_kernel(
    unsigned short* __restrict__ out_bf16,    // [M, N] (splits == 1)
    float* __restrict__ ws,                   // [S, M, N] (splits > 1)
    const unsigned short* __restrict__ x,     // [M, K] bf16
    const unsigned char* __restrict__ wp,     // [N, K/2] packed nibbles
    const unsigned short* __restrict__ sc,    // [N, K/128] bf16
    const unsigned char* __restrict__ zp,     // [N, K/128]
    int M, int N, int K) {
  // ---- block -> (m0, n0): XCD x takes a contiguous run of tiles ----
  const int mt = (M + PS_W4T_BM - 1) / PS_W4T_BM;
  const int nwg = mt * ((N + PS_W4T_BN - 1) / PS_W4T_BN);
  int wg;
  {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = blockIdx.x & 7, lin = blockIdx.x >> 3;
    if (lin >= (xcd < r ? q + 1 : q)) return;  // padding of the grid
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lin;
  }
  const int m0 = (wg % mt) * PS_W4T_BM;
  const int n0 = (wg / mt) * PS_W4T_BN;

  const int kgroups = K / PS_W4_GROUP;
  const auto [kc_begin, kc_end] =
      ps_split_range_of(kgroups, gridDim.y, blockIdx.y);
  if (kc_begin >= kc_end) return;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int g = lane >> 4;   // k-group of a frag
  const int rc = lane & 15;  // row (A) / col (B, C) within a 16-tile
  const int wm = wave >> 1;  // wave M position (2)
  const int wn = wave & 1;   // wave N position (2)
  // whether any of the wave's 64 x 64 outputs exist (N % 64 == 0)
  const bool live = m0 + wm * 64 < M && n0 + wn * 64 < N;

  __shared__ __align__(16) unsigned short a_lds[PS_W4T_BM][PS_W4_GROUP];
  __shared__ __align__(16) unsigned short b_lds[PS_W4T_BN][PS_W4_GROUP];

  // ---- staging registers of one group and who fills them ----
  const int wrow = tid >> 2;  // W rows wrow and wrow + 64
  const int wg4 = tid & 3;    // lane group g of the packed layout
  const int xrow = tid >> 4;  // x rows xrow + 16 i
  const int xslot = tid & 15;
  ps_w4u32x4 wq[2];
  unsigned short s_raw[2];
  unsigned char z_raw[2];
  ps_bf16x8 xv[8];

  // Rows past the M or N edge load the last valid row instead of branching
  // around the load: C[m][n] depends on x row m and W row n alone, and no
  // such m or n is stored.
  auto load = [&](int c) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const long n = min(n0 + wrow + 64 * h, N - 1);
      wq[h] = *(const ps_w4u32x4*)(wp + n * (K / 2) + (long)c * 64 +
                                   wg4 * 16);
      s_raw[h] = sc[n * kgroups + c];
      z_raw[h] = zp[n * kgroups + c];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const long m = min(m0 + xrow + 16 * i, M - 1);
      xv[i] = *(const ps_bf16x8*)(x + m * K + (long)c * PS_W4_GROUP +
                                  xslot * 8);
    }
  };

  auto store = [&]() {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int row = wrow + 64 * h;
      const float s = ps_bf16_to_f32(s_raw[h]);
      const float nzs = -((float)z_raw[h] * s);
#pragma unroll
      for (int j = 0; j < 4; j++)
        *(ps_mfma_bf16x8*)(&b_lds[row][((4 * j + wg4) ^ (row & 15)) * 8]) =
            ps_w4_dequant8(wq[h][j], s, nzs);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int row = xrow + 16 * i;
      *(ps_bf16x8*)(&a_lds[row][(xslot ^ (row & 15)) * 8]) = xv[i];
    }
  };

  ps_f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  load(kc_begin);
  store();
  __syncthreads();
  for (int kc = kc_begin;; kc++) {
    const bool more = kc + 1 < kc_end;  // uniform over the workgroup
    if (more) load(kc + 1);
    if (live) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int slot = ((4 * j + g) ^ rc) * 8;  // row & 15 == rc
        ps_mfma_bf16x8 af[4], bf[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          af[t] = *(const ps_mfma_bf16x8*)(
              &a_lds[wm * 64 + t * 16 + rc][slot]);
          bf[t] = *(const ps_mfma_bf16x8*)(
              &b_lds[wn * 64 + t * 16 + rc][slot]);
        }
#pragma unroll
        for (int mtl = 0; mtl < 4; mtl++)
#pragma unroll
          for (int ntl = 0; ntl < 4; ntl++)
            acc[mtl][ntl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[mtl], bf[ntl], acc[mtl][ntl], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    if (!more) break;
    __syncthreads();  // every wave has read group kc
    store();
    __syncthreads();  // group kc + 1 is in LDS
  }

  // ---- epilogue (C layout: row = g*4 + r, col = rc of each 16x16 tile) ----
  // A lone split writes the bf16 output; otherwise each split streams its
  // fp32 partial to ws[split][M][N] for the combine kernel.
  if (!live) return;
  const bool lone = gridDim.y == 1;
  const int mrow = m0 + wm * 64 + g * 4;
  const long col = n0 + wn * 64 + rc;
  float* part = ws + (long)blockIdx.y * M * N;
#pragma unroll
  for (int mtl = 0; mtl < 4; mtl++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = mrow + mtl * 16 + r;
      if (m >= M) continue;
      const long at = (long)m * N + col;
#pragma unroll
      for (int ntl = 0; ntl < 4; ntl++) {
        if (lone)
          out_bf16[at + ntl * 16] = ps_f32_to_bf16(acc[mtl][ntl][r]);
        else
          part[at + ntl * 16] = acc[mtl][ntl][r];
      }
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" {

// Split depth for a shape; -1 if unsupported. Every weight quantize_int4
// produces is supported at every M >= 1.
int ps_gemm_w4_tiled_splits(int M, int N, int K) {
  if (M < 1 || N < 64 || K < PS_W4_GROUP || N % 64 != 0 ||
      K % PS_W4_GROUP != 0)
    return -1;
  const long tiles = (long)ps_cdiv(M, PS_W4T_BM) * ps_cdiv(N, PS_W4T_BN);
  if (tiles >= PS_W4T_TARGET_WGS) return 1;
  return ps_splitk_depth(K / PS_W4_GROUP, (int)tiles, PS_W4T_TARGET_WGS, 1);
}

// ws == nullptr forces splits = 1.
int ps_gemm_w4_tiled(void* out_bf16, void* ws, const void* x,
                     const void* packed, const void* scales,
                     const void* zeros, int M, int N, int K,
                     hipStream_t stream) {
  int splits = ps_gemm_w4_tiled_splits(M, N, K);
  if (splits < 0) return -1;
  if (ws == nullptr) splits = 1;
  const long tiles = (long)ps_cdiv(M, PS_W4T_BM) * ps_cdiv(N, PS_W4T_BN);
  if (tiles > 0x7ffffff0L) return -1;
  dim3 grid((unsigned)((tiles + 7) / 8 * 8), splits);
  gemm_w4_tiled_kernel<<<grid, 256, 0, stream>>>(
      (unsigned short*)out_bf16, splits > 1 ? (float*)ws : nullptr,
      (const unsigned short*)x, (const unsigned char*)packed,
      (const unsigned short*)scales, (const unsigned char*)zeros, M, N, K);
  if (splits > 1)
    ps_launch_splitk_combine(out_bf16, ws, M, N, splits, stream);
  return 0;
}

}  // extern "C"
