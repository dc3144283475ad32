// Fused sparse-MoE expert MLP with int4 weight-only (W4A16) experts: the
// contract of moe_fused.hip,
//   out[t] = sum_k w[t,k] * down_e( silu(gate_e(x[t])) * up_e(x[t]) ),
//   e = topk_ids[t,k], bf16 activations, fp32 accumulation,
// on expert weights in the packed format of skinny_gemm_w4.hip (group 128
// along K, W_deq = bf16_rne((q - z) * s), nibble order of ops.int4_pack).
// The MFMA operands are exactly the W_deq bf16 values. A stacked expert
// tensor [E, N, K/2] is the packed [E*N, K/2] matrix, reshaped.
//
// MoE decode is weight-bandwidth-bound; int4 cuts the expert bytes ~3.9x
// (64 B + 2 B scale + 1 B zero point per 128 weights).
//
//   moe_align        csrc/moe_common.h, shared with moe_fused.hip.
//   moe_grouped_w4   grid (N/64, E, S): moe_fused.hip's grouping with
//                    skinny_gemm_w4.hip's main loop. A workgroup owns 64
//                    weight rows of expert e (GATED: 64 gate rows + the
//                    matching 64 up rows) over a K-range of 128-wide groups,
//                    and streams them once per 16*M_TILES-row chunk of the
//                    expert's pairs. 4 waves x 16 rows, a lane reads its own
//                    row: one 16-B load per group is the four B-fragments of
//                    that group with no cross-lane move. An iteration covers
//                    up to CPI groups: packed loads, s and z of all of them
//                    are issued first, then the activation rows are gathered
//                    into LDS, then each group is dequantized in registers
//                    and runs 4 MFMAs per m-tile per branch, groups in
//                    ascending k. Experts with no pairs return before any
//                    barrier.
//                    GATED (S = 1): act[p] = silu(g) * u in fp32 -> bf16.
//                    else: y[split][p] = fp32 partial down-projection rows.
//   moe_combine_w4   out[t] = sum_k w[t,k] * (sum_s y[s][t*top_k+k]), s then
//                    k ascending, one pass, no atomics.
//
// Down GEMM split-K over I: a workgroup's int4 stream is 4x shorter than the
// bf16 kernel's, and H/64 workgroups per routed expert leave most CUs idle at
// small T. S = ps_fused_moe_w4_splits(top_k, H, I) is a function of the
// model shape only, never of T or the routing: launch shapes stay capturable
// and a pair's result does not depend on the batch it rides in. Every
// M_TILES instantiation accumulates group by group in the same order, so the
// output row of a token is bit-identical at any T. A split of a non-empty
// expert never has an empty K-range (ps_splitk_depth's fixed point with
// ps_split_range_of's partition), so every y row the combine reads was
// written by every split.
//
// LDS: a_lds[CPI][MP][128] bf16 with skinny_gemm_w4.hip's 16-slot XOR swizzle
// (slot ^ (row & 15)), at most 2 * 64 * 256 B = 32 KiB, single-buffered.
// Barriers per iteration: one after the gather (every writer of a_lds is done
// before any MFMA operand read), one after the MFMAs (every reader is done
// before the next iteration's gather overwrites a_lds). pair_lds / arow_lds
// are rewritten per chunk between two barriers of their own: the first keeps
// the previous chunk's epilogue readers ahead of the write, the second puts
// the write ahead of the gather.
#include "moe_common.h"
#include "w4_common.h"

#define PS_MOE_W4_MAX_SPLITS 8  // y stays <= 8 * P * H * 4 B

// GATED:  a = x[T, K=H],   weight rows [E, 2N, .], N = I,
//         out_act[P, N] bf16 = silu(a.Wg^T) * (a.Wu^T); A row = pair/top_k.
// !GATED: a = act[P, K=I], weight rows [E, N, .],  N = H,
//         out_y[S, P, N] fp32 partials = a.W^T over the split's K-range;
//         A row = pair.
template <int M_TILES, int CPI, bool GATED>
__global__ __launch_bounds__(256) void moe_grouped_w4_kernel(
    unsigned short* __restrict__ out_act, float* __restrict__ out_y,
    const unsigned short* __restrict__ a,
    const unsigned char* __restrict__ wp,   // [E, NB*N, K/2] packed nibbles
    const unsigned short* __restrict__ sc,  // [E, NB*N, K/128] bf16
    const unsigned char* __restrict__ zp,   // [E, NB*N, K/128]
    const int* __restrict__ offsets, const int* __restrict__ sorted_pairs,
    int top_k, int P, int N, int K) {
  constexpr int MP = M_TILES * 16;  // rows per chunk
  constexpr int NB = GATED ? 2 : 1;
  const int e = blockIdx.y;
  const int row0 = offsets[e];
  const int count = offsets[e + 1] - row0;  // workgroup-uniform
  if (count <= 0) return;
  const int kgroups = K / PS_W4_GROUP;
  const auto [kc_begin, kc_end] =
      ps_split_range_of(kgroups, gridDim.z, blockIdx.z);
  // never taken: csrc/tools/splitk_check.cpp sweeps ps_splitk_depth_capped
  // (round_to 4, at most 8 splits) for "every split owns a group"; taken, it
  // would leave this split's y slice unwritten under the combine
  if (kc_begin >= kc_end) return;

  const int tid = threadIdx.x;
  const auto [wave, g, rc, nrow] = ps_skinny_lane_of();
  // branch b = 0 is the gate (or the only) row, b = 1 the up row I + nrow
  const long wrow0 = (long)e * NB * N + nrow;
  const unsigned char* wrow[NB];
  const unsigned short* srow[NB];
  const unsigned char* zrow[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    const long r = wrow0 + (long)b * N;
    wrow[b] = wp + r * (K / 2) + g * 16;
    srow[b] = sc + r * kgroups;
    zrow[b] = zp + r * kgroups;
  }

  __shared__ __align__(16) unsigned short a_lds[CPI][MP][PS_W4_GROUP];
  __shared__ int pair_lds[MP];  // pair id of each chunk row, -1 past count
  __shared__ int arow_lds[MP];  // its row of a, -1 past count

  for (int c0 = 0; c0 < count; c0 += MP) {
    __syncthreads();  // previous chunk's readers of pair_lds / arow_lds done
    if (tid < MP) {
      const int r = c0 + tid;
      const int pr = r < count ? sorted_pairs[row0 + r] : -1;
      pair_lds[tid] = pr;
      arow_lds[tid] = pr < 0 ? -1 : (GATED ? pr / top_k : pr);
    }
    __syncthreads();

    ps_f32x4 acc[NB][M_TILES];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
      for (int mt = 0; mt < M_TILES; mt++) acc[b][mt] = {0.f, 0.f, 0.f, 0.f};

    for (int kc = kc_begin; kc < kc_end; kc += CPI) {
      const int nc = min(CPI, kc_end - kc);  // groups this iteration
      // ---- packed W first: rows streamed once per chunk ----
      ps_w4u32x4 wq[NB][CPI];
      float s[NB][CPI], nzs[NB][CPI];
#pragma unroll
      for (int b = 0; b < NB; b++) {
#pragma unroll
        for (int c = 0; c < CPI; c++) {
          wq[b][c] = {0u, 0u, 0u, 0u};
          s[b][c] = 0.f;
          nzs[b][c] = 0.f;
          if (c < nc) {
            wq[b][c] = *(const ps_w4u32x4*)(wrow[b] + (long)(kc + c) * 64);
            s[b][c] = ps_bf16_to_f32(srow[b][kc + c]);
            nzs[b][c] = -((float)zrow[b][kc + c] * s[b][c]);
          }
        }
      }
      // ---- activation gather: nc*MP*16 16-B slots over 256 threads ----
      for (int u = tid; u < nc * MP * 16; u += 256) {
        const int c = u / (MP * 16);
        const int row = (u >> 4) & (MP - 1);
        const int slot = u & 15;
        const int arow = arow_lds[row];
        ps_bf16x8 v = {};
        if (arow >= 0)
          v = *(const ps_bf16x8*)(a + (long)arow * K +
                                  (long)(kc + c) * PS_W4_GROUP + slot * 8);
        *(ps_bf16x8*)(&a_lds[c][row][(slot ^ (row & 15)) * 8]) = v;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < CPI; c++) {
        if (c < nc) {
          // ---- B-frags built in registers ----
          ps_mfma_bf16x8 bf[NB][4];
#pragma unroll
          for (int b = 0; b < NB; b++)
#pragma unroll
            for (int j = 0; j < 4; j++)
              bf[b][j] = ps_w4_dequant8(wq[b][c][j], s[b][c], nzs[b][c]);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int mt = 0; mt < M_TILES; mt++) {
            const int row = mt * 16 + rc;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const ps_mfma_bf16x8 av = *(const ps_mfma_bf16x8*)(
                  &a_lds[c][row][((4 * j + g) ^ (row & 15)) * 8]);
#pragma unroll
              for (int b = 0; b < NB; b++)
                acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    av, bf[b][j], acc[b][mt], 0, 0, 0);
            }
          }
          __builtin_amdgcn_s_setprio(0);
        }
      }
      __syncthreads();
    }

    // ---- epilogue (C layout: row=(g*4+r), col=rc of each 16x16 tile)
#pragma unroll
    for (int mt = 0; mt < M_TILES; mt++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = mt * 16 + g * 4 + r;
        if (c0 + m >= count) continue;
        const long pr = pair_lds[m];
        if (GATED) {
          const float gv = acc[0][mt][r];
          const float uv = acc[NB - 1][mt][r];
          const float sg = gv / (1.f + __expf(-gv));
          out_act[pr * N + nrow] = ps_f32_to_bf16(sg * uv);
        } else {
          out_y[((long)blockIdx.z * P + pr) * N + nrow] = acc[0][mt][r];
        }
      }
    }
  }
}

// out[t, h0..h0+3] = sum_k w[t,k] * (sum_s y[s, t*top_k+k, h0..h0+3]); one
// thread per 4 columns, s ascending inside k ascending (fixed order).
__global__ __launch_bounds__(256) void moe_combine_w4_kernel(
    unsigned short* __restrict__ out,  // [T, H] bf16
    const float* __restrict__ y,       // [S, T*top_k, H] fp32
    const float* __restrict__ topk_w,  // [T, top_k] fp32
    int T, int top_k, int H, int splits) {
  const int hq = H / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)T * hq) return;
  const int t = (int)(i / hq);
  const int h0 = (int)(i % hq) * 4;
  const long PH = (long)T * top_k * H;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < top_k; k++) {
    const float wk = topk_w[t * top_k + k];
    const float* yk = y + ((long)t * top_k + k) * H + h0;
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; s++) {
      const ps_f32x4 v = *(const ps_f32x4*)(yk + s * PH);
#pragma unroll
      for (int j = 0; j < 4; j++) part[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = __builtin_fmaf(wk, part[j], acc[j]);
  }
  ps_bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = ps_f32_to_bf16(acc[j]);
  *(ps_bf16x4*)(out + (long)t * H + h0) = o;
}

extern "C" {

// The accept rule; ops.fused_moe_int4_supported mirrors it.
int ps_fused_moe_w4_supported(int T, int top_k, int E, int H, int I) {
  if (T < 1 || top_k < 1 || E < 1 || H < PS_W4_GROUP || I < PS_W4_GROUP)
    return 0;
  if (E > PS_MOE_MAX_EXPERTS || top_k > E) return 0;
  if ((long)T * top_k > PS_MOE_MAX_PAIRS) return 0;
  if (H % PS_W4_GROUP != 0 || I % PS_W4_GROUP != 0) return 0;
  return 1;
}

// Split depth of the down GEMM, a function of the model shape only; -1 if
// unsupported. At T = 1 the down GEMM launches (H/64) * top_k workgroups per
// split with work to do; the depth aims for 1024 of them (4 per CU), at most
// PS_MOE_W4_MAX_SPLITS, in whole PS_W4_MAX_CPI-group iterations.
int ps_fused_moe_w4_splits(int top_k, int H, int I) {
  if (top_k < 1 || H < PS_W4_GROUP || I < PS_W4_GROUP ||
      H % PS_W4_GROUP != 0 || I % PS_W4_GROUP != 0)
    return -1;
  const long wgs = (long)(H / 64) * top_k;
  if (wgs > 1024) return 1;
  return ps_splitk_depth_capped(I / PS_W4_GROUP, (int)wgs, 1024,
                                PS_W4_MAX_CPI, PS_MOE_W4_MAX_SPLITS);
}

// Scratch (every element that is later read is overwritten first, no
// initialisation needed):
//   offsets int32[E+1], sorted_pairs int32[T*top_k],
//   act bf16[T*top_k, I], y fp32[S, T*top_k, H], S = ps_fused_moe_w4_splits.
// gu_* are the gate_up triple ([E, 2I, H/2], [E, 2I, H/128] x2), dn_* the
// down triple ([E, H, I/2], [E, H, I/128] x2).
int ps_fused_moe_w4(void* out, void* offsets, void* sorted_pairs, void* act,
                    void* y, const void* x, const void* gu_packed,
                    const void* gu_s, const void* gu_z, const void* dn_packed,
                    const void* dn_s, const void* dn_z, const void* topk_ids,
                    int ids_i64, const void* topk_w, int T, int top_k, int E,
                    int H, int I, hipStream_t stream) {
  if (!ps_fused_moe_w4_supported(T, top_k, E, H, I)) return -1;
  const int P = T * top_k;
  const int splits = ps_fused_moe_w4_splits(top_k, H, I);
  ps_launch_moe_align(offsets, sorted_pairs, topk_ids, ids_i64, P, E, stream);
  // an expert receives each token at most once, so count <= T
#define PS_MOE_W4(MT, GATED, S, N, K, A, WP, WS, WZ)                        \
  moe_grouped_w4_kernel<MT, ps_w4_cpi(MT), GATED>                           \
      <<<dim3((N) / 64, E, S), 256, 0, stream>>>(                           \
          (unsigned short*)act, (float*)y, (const unsigned short*)(A),      \
          (const unsigned char*)(WP), (const unsigned short*)(WS),          \
          (const unsigned char*)(WZ), (const int*)offsets,                  \
          (const int*)sorted_pairs, top_k, P, N, K)
#define PS_MOE_W4_PAIR(MT)                                                  \
  do {                                                                      \
    PS_MOE_W4(MT, true, 1, I, H, x, gu_packed, gu_s, gu_z);                 \
    PS_MOE_W4(MT, false, splits, H, I, act, dn_packed, dn_s, dn_z);         \
  } while (0)
  if (T <= 16)
    PS_MOE_W4_PAIR(1);
  else if (T <= 32)
    PS_MOE_W4_PAIR(2);
  else
    PS_MOE_W4_PAIR(4);
#undef PS_MOE_W4_PAIR
#undef PS_MOE_W4
  const long n4 = (long)T * (H / 4);
  moe_combine_w4_kernel<<<dim3((unsigned)((n4 + 255) / 256)), 256, 0,
                          stream>>>(
      (unsigned short*)out, (const float*)y, (const float*)topk_w, T, top_k,
      H, splits);
  return 0;
}

}  // extern "C"
