// fp8 GEMM tiled in M and N, for prefill-sized steps:
//   out[M, N] bf16 = (xq[M, K] * sx[M, None]) @ (wq[N, K] * sw[N, None])^T
// xq / wq OCP e4m3, sx / sw fp32, fp32 accumulation, any M >= 1.
// Format and numerics are skinny_gemm_fp8.hip's: unscaled fp32 sums,
// sx[m] * sw[n] formed in fp32 and applied once right before the bf16 round
// (GEMM epilogue for one split, combine kernel otherwise), no atomics. That
// kernel streams W once and re-reads x from LDS for every MFMA, which is right
// while W dominates the traffic (M <= 256); here both operands are staged in
// LDS tiles and reused from registers. The tiling is gemm_w4_tiled.hip's, but
// fp8 needs no transform between the global load and LDS, so the LDS images
// are double-buffered and a k-step costs one barrier.
//
// Plan:
//   Tile 128 (M) x 128 (N) per workgroup, 256 threads, waves 2 x 2, each
//   owning 64 x 64 = 4 x 4 MFMA tiles (64 accumulator VGPRs).
//   K step = 128 fp8 = 128 B per row. The A image is [128][128 B], the B
//   image the same: 1024 16-B slots per operand, four 16-B loads per thread
//   per operand (slot t%8, rows t/8 + 32i; 8 consecutive lanes read one
//   128-B row segment). Two stages of both images = 64 KiB, so two
//   workgroups fit a CU's 160 KiB.
//   Pipeline: the global loads of k-step c+1 are issued into registers before
//   the MFMAs of step c and written to the other LDS stage after them; one
//   barrier per k-step. Stage X is read in step c-1 and overwritten in step
//   c after the barrier that ends c-1, which every wave reaches with its
//   reads of X complete; it is read again in step c+1 after the barrier that
//   ends c, which every wave reaches with its writes done.
//   A final half k-step (K % 128 == 64) zero-fills slots 4..7 in LDS instead
//   of loading them; fp8 zero bytes are 0.0.
//   MFMA: v_mfma_f32_16x16x128_f8f6f4 (both formats e4m3, no block scales),
//   16 per wave per k-step from 4 + 4 fragments of two ds_read_b128 each.
//   Lane (g, rc) feeds bytes [32g, 32g+32) of its A row and of its B row. A
//   and B use the same k offsets, so whatever order the instruction gives
//   its 128 k, the sum pairs x[m][k] with w[n][k]; only the row/col lane map
//   (lane & 15) and the C/D map (col = lane & 15, row = 4*(lane>>4) + r)
//   matter. template DEEP = false issues four mfma_f32_16x16x32_fp8_fp8 on
//   the same registers instead (bytes [32g+8j, 32g+8j+8) to the j-th);
//   csrc/tools/gemm_fp8_tiled_ab.hip times both forms. On an MI355X, one
//   split, median of 7 alternating windows (min..max):
//     M=4096 N=28672 K=4096: 128-deep 648.9 us (646.9..666.6), 1483 TFLOP/s;
//                            4 x 32-deep 925.2 us (897.6..977.1), 1040 TFLOP/s
//     M=4096 N=4096  K=4096: 128-deep 92.9 us (91.3..103.5), 1480 TFLOP/s;
//                            4 x 32-deep 144.0 us (140.5..170.4), 954 TFLOP/s
//   so the 128-deep form is the one launched (PS_F8T_DEEP). It also needs
//   188 VGPRs against 220.
//
// LDS swizzle: rows are 128 B = 8 16-B slots, so rows 2p and 2p+1 share a
// 256-B bank row, row r at positions 8(r&1) + slot. ds_read_b128 is served in
// 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32 for the upper
// half; see skinny_gemm_fp8.hip). With q = (rc>>2)&3 and e = (q ^ q>>1) & 1,
// a group holds the rows with e == 0 at one g and those with e == 1 at the
// other, g in {a, a+1}, a in {0, 2}. The first fragment read is at logical
// slot 2g, so within a group the slot is a constant XOR (0, e, 0) in bits
// (2, 1, 0). The 8 even rows of a group (the odd ones likewise, in the other
// half of the bank row) are told apart by (q1, q0, b), b = (rc>>1)&1, and
// must land on 8 different slots. Storing slot s of row r at s ^ f(r) with
//   f = (q1, q1, b) = 6 * ((r>>3)&1) | ((r>>1)&1)
// gives slot bits const ^ (q1, e ^ q1, b) = const ^ (q1, q0, b): a bijection
// of the 8 rows onto the 8 slots, so the 16 lanes cover the bank row:
// conflict-free. The second read, slot 2g+1, is the same with bit 0 flipped.
// (No XOR puts the four rows of one q pair-wise on one slot: 4-way.) f reads
// bits 1 and 3 of the row only, so the 16-row tile offsets do not change it.
// The staging ds_write_b128 goes in groups of 8 consecutive lanes = the 8
// slots of one row, one 128-B span under any XOR within the row:
// conflict-free under its 32-bank rule.
//
//   Tails: an x row >= M, or a W row >= N of the 64-row last tile that
//   N % 128 == 64 leaves, reads the last valid row in its place and is never
//   stored (gemm_w4_tiled.hip's rule and reasoning). Waves whose 64 x 64
//   block lies wholly past an edge skip their MFMAs.
//   Grid = (tiles rounded up to 8, splits); tiles are numbered M-fastest
//   behind gemm_w4_tiled's bijective XCD remap. Split-K over whole k-steps
//   for launches that would leave CUs idle: unscaled fp32 partials to
//   ws[S, M, N], summed in split order and scaled by the fp8 combine kernel
//   (fp8_common.h). Bit-deterministic for a fixed (M, N, K); the depth depends
//   on the tile count, so unlike skinny_gemm_fp8 a row's bits may depend on M.
//
// Compiler resource summary (gfx950, the launched 128-deep form): 188 VGPRs,
// 0 AGPRs, 39 SGPRs, 65536 B LDS, 0 B scratch, occupancy 2 waves per SIMD,
// i.e. two workgroups per CU by both LDS and registers.
#include "fp8_common.h"

// No packed-fp32 VALU ops (v_pk_mul_f32 and kin) in this file's device code:
// the epilogue's scale products are emitted as scalar multiplies instead.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                  \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

typedef __attribute__((ext_vector_type(4))) int ps_f8t_i32x4;  // 16 fp8
typedef __attribute__((ext_vector_type(8))) int ps_f8t_i32x8;  // 32 fp8

#define PS_F8T_BM 128
#define PS_F8T_BN 128
#define PS_F8T_BK 128  // fp8 per row per k-step

// Workgroups resident at once, the grid size split-K aims for: 256 CUs x 2
// workgroups per CU (LDS: 64 KiB each of 160 KiB).
#define PS_F8T_TARGET_WGS 512

// slot XOR of a row of an LDS image (see the header)
PS_DEV int ps_f8t_swz(int row) {
  return ((row >> 3) & 1) * 6 | ((row >> 1) & 1);
}

// __syncthreads() written out: under this file's target attribute the
// library function is not inlined into the kernel and every barrier becomes a
// call.
PS_DEV void ps_f8t_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool DEEP>
__global__ __launch_bounds__(256, 2) void gemm_fp8_tiled_kernel(
    unsigned short* __restrict__ out_bf16,  // [M, N] (splits == 1)
    float* __restrict__ ws,                 // [S, M, N] (splits > 1)
    const unsigned char* __restrict__ xq,   // [M, K] e4m3
    const float* __restrict__ sx,           // [M]
    const unsigned char* __restrict__ wq,   // [N, K] e4m3
    const float* __restrict__ sw,           // [N]
    int M, int N, int K) {
  // ---- block -> (m0, n0): XCD x takes a contiguous run of tiles ----
  const int mt = (M + PS_F8T_BM - 1) / PS_F8T_BM;
  const int nwg = mt * ((N + PS_F8T_BN - 1) / PS_F8T_BN);
  int wg;
  {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = blockIdx.x & 7, lin = blockIdx.x >> 3;
    if (lin >= (xcd < r ? q + 1 : q)) return;  // padding of the grid
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lin;
  }
  const int m0 = (wg % mt) * PS_F8T_BM;
  const int n0 = (wg / mt) * PS_F8T_BN;

  const auto [kc_begin, kc_end] = ps_split_range_of(
      (K + PS_F8T_BK - 1) / PS_F8T_BK, gridDim.y, blockIdx.y);
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

  __shared__ __align__(16) unsigned char a_lds[2][PS_F8T_BM][PS_F8T_BK];
  __shared__ __align__(16) unsigned char b_lds[2][PS_F8T_BN][PS_F8T_BK];

  // ---- staging registers of one k-step and who fills them ----
  const int srow = tid >> 3;  // rows srow + 32 i of both images
  const int sslot = tid & 7;
  // Rows past the M or N edge load the last valid row instead of branching
  // around the load: C[m][n] depends on x row m and W row n alone, and no
  // such m or n is stored.
  const unsigned char* ap[4];
  const unsigned char* bp[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    ap[i] = xq + (long)min(m0 + srow + 32 * i, M - 1) * K + sslot * 16;
    bp[i] = wq + (long)min(n0 + srow + 32 * i, N - 1) * K + sslot * 16;
  }
  ps_f8t_i32x4 av[4], bv[4];

  auto load = [&](int c) {
    const long k = (long)c * PS_F8T_BK;
    // false only for slots 4..7 of a final half k-step
    if (k + sslot * 16 < K) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        av[i] = *(const ps_f8t_i32x4*)(ap[i] + k);
        bv[i] = *(const ps_f8t_i32x4*)(bp[i] + k);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        av[i] = {0, 0, 0, 0};
        bv[i] = {0, 0, 0, 0};
      }
    }
  };

  // bits 1 and 3 of srow + 32 i are srow's
  const int sat = (sslot ^ ps_f8t_swz(srow)) * 16;
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      *(ps_f8t_i32x4*)(&a_lds[buf][srow + 32 * i][sat]) = av[i];
      *(ps_f8t_i32x4*)(&b_lds[buf][srow + 32 * i][sat]) = bv[i];
    }
  };

  ps_f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // bytes [32g, 32g+32) of row rc: slots 2g and 2g+1, swizzled
  const int fat = ((2 * g) ^ ps_f8t_swz(rc)) * 16;

  load(kc_begin);
  store(0);
  ps_f8t_barrier();
  for (int kc = kc_begin;; kc++) {
    const int cur = (kc - kc_begin) & 1;
    const bool more = kc + 1 < kc_end;  // uniform over the workgroup
    if (more) load(kc + 1);
    if (live) {
      ps_f8t_i32x8 af[4], bf[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const unsigned char* pa = &a_lds[cur][wm * 64 + t * 16 + rc][0];
        const unsigned char* pb = &b_lds[cur][wn * 64 + t * 16 + rc][0];
        const ps_f8t_i32x4 a0 = *(const ps_f8t_i32x4*)(pa + fat);
        const ps_f8t_i32x4 a1 = *(const ps_f8t_i32x4*)(pa + (fat ^ 16));
        const ps_f8t_i32x4 b0 = *(const ps_f8t_i32x4*)(pb + fat);
        const ps_f8t_i32x4 b1 = *(const ps_f8t_i32x4*)(pb + (fat ^ 16));
        af[t] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        bf[t] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mtl = 0; mtl < 4; mtl++)
#pragma unroll
        for (int ntl = 0; ntl < 4; ntl++) {
          if constexpr (DEEP) {
            acc[mtl][ntl] =
                __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                    af[mtl], bf[ntl], acc[mtl][ntl], 0, 0, 0, 0, 0, 0);
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const long a8 = (long)(unsigned)af[mtl][2 * j] |
                              ((long)af[mtl][2 * j + 1] << 32);
              const long b8 = (long)(unsigned)bf[ntl][2 * j] |
                              ((long)bf[ntl][2 * j + 1] << 32);
              acc[mtl][ntl] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                  a8, b8, acc[mtl][ntl], 0, 0, 0);
            }
          }
        }
      __builtin_amdgcn_s_setprio(0);
    }
    if (!more) break;
    store(cur ^ 1);
    ps_f8t_barrier();  // step kc + 1 is in LDS; every wave has read step kc
  }

  // ---- epilogue (C layout: row = g*4 + r, col = rc of each 16x16 tile) ----
  // A lone split scales and writes the bf16 output; otherwise each split
  // streams its unscaled fp32 partial to ws[split][M][N] for the combine.
  if (!live) return;
  const bool lone = gridDim.y == 1;
  const int mrow = m0 + wm * 64 + g * 4;
  const long col = n0 + wn * 64 + rc;
  float* part = ws + (long)blockIdx.y * M * N;
  float swn[4];
#pragma unroll
  for (int ntl = 0; ntl < 4; ntl++) swn[ntl] = lone ? sw[col + ntl * 16] : 0.f;
#pragma unroll
  for (int mtl = 0; mtl < 4; mtl++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = mrow + mtl * 16 + r;
      if (m >= M) continue;
      const long at = (long)m * N + col;
      if (lone) {
        const float sxm = sx[m];
#pragma unroll
        for (int ntl = 0; ntl < 4; ntl++)
          out_bf16[at + ntl * 16] =
              ps_f32_to_bf16(acc[mtl][ntl][r] * (sxm * swn[ntl]));
      } else {
#pragma unroll
        for (int ntl = 0; ntl < 4; ntl++)
          part[at + ntl * 16] = acc[mtl][ntl][r];
      }
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// The MFMA form ps_gemm_fp8_tiled launches (see the header for the A/B)
#define PS_F8T_DEEP true

// Split depth for a shape; -1 if unsupported. skinny_gemm_fp8's accept rule
// without the M cap.
static inline int ps_f8t_splits(int M, int N, int K) {
  if (M < 1 || N < 64 || K < 64 || N % 64 != 0 || K % 64 != 0) return -1;
  const long tiles = (long)ps_cdiv(M, PS_F8T_BM) * ps_cdiv(N, PS_F8T_BN);
  if (tiles >= PS_F8T_TARGET_WGS) return 1;
  return ps_splitk_depth(ps_cdiv(K, PS_F8T_BK), (int)tiles,
                         PS_F8T_TARGET_WGS, 1);
}

// ws == nullptr forces splits = 1.
template <bool DEEP>
static int ps_f8t_launch(void* out_bf16, void* ws, const void* xq,
                         const void* sx, const void* wq, const void* sw,
                         int M, int N, int K, hipStream_t stream) {
  int splits = ps_f8t_splits(M, N, K);
  if (splits < 0) return -1;
  if (ws == nullptr) splits = 1;
  const long tiles = (long)ps_cdiv(M, PS_F8T_BM) * ps_cdiv(N, PS_F8T_BN);
  if (tiles > 0x7ffffff0L) return -1;
  dim3 grid((unsigned)((tiles + 7) / 8 * 8), splits);
  gemm_fp8_tiled_kernel<DEEP><<<grid, 256, 0, stream>>>(
      (unsigned short*)out_bf16, splits > 1 ? (float*)ws : nullptr,
      (const unsigned char*)xq, (const float*)sx, (const unsigned char*)wq,
      (const float*)sw, M, N, K);
  if (splits > 1)
    ps_launch_fp8_combine(out_bf16, ws, sx, sw, M, N, splits, stream);
  return 0;
}

extern "C" {

int ps_gemm_fp8_tiled_splits(int M, int N, int K) {
  return ps_f8t_splits(M, N, K);
}

int ps_gemm_fp8_tiled(void* out_bf16, void* ws, const void* xq,
                      const void* sx, const void* wq, const void* sw, int M,
                      int N, int K, hipStream_t stream) {
  return ps_f8t_launch<PS_F8T_DEEP>(out_bf16, ws, xq, sx, wq, sw, M, N, K,
                                    stream);
}

}  // extern "C"
