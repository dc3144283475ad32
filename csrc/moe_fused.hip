// Fused sparse-MoE expert MLP for decode-shaped batches (Mixtral family):
//   out[t] = sum_k w[t,k] * down_e( silu(gate_e(x[t])) * up_e(x[t]) ),
//   e = topk_ids[t,k], bf16 weights/activations, fp32 accumulation.
//
// Why it exists: the per-expert Python loop costs a host sync + ~6 launches
// per expert and its row gathers make the launch sequence depend on the
// routing, which rules out hipGraph capture. Here every launch has a grid
// that depends only on (T, top_k, E, H, I); the routing is consumed on the
// device, there is no host readback and no atomics, so the sequence is
// capturable and bit-deterministic.
//
//   moe_align       1 workgroup: counting sort of the T*top_k (token,k)
//                   pairs by expert -> expert_offsets[E+1], sorted_pairs[P]
//                   (stable: pairs keep ascending order inside an expert).
//   moe_grouped     grid (N/64, E): the skinny_gemm structure, grouped.
//                   A workgroup owns 64 weight rows of expert e (gate_up: 64
//                   gate rows + the matching 64 up rows), streams them once
//                   per 16*M_TILES-row chunk of the expert's pairs, gathers
//                   the activation rows on the device into XOR-swizzled
//                   LDS. Experts with no pairs return before any barrier.
//                   GATED: act[p] = silu(g) * u in fp32 -> bf16.
//                   else : y[p]   = fp32 down-projection rows.
//   moe_combine     out[t] = sum_k w[t,k] * y[t*top_k+k], fixed k order.
// mfma_f32_16x16x32_bf16; operand k-pattern as verified in
// csrc/tools/mfma_probe.hip.
#include "skinny_common.h"

#define PS_MOE_MAX_PAIRS 1024
#define PS_MOE_MAX_EXPERTS 64

// One workgroup of 1024 threads, thread p owns pair p = t*top_k + k.
// Per wave, a ballot per expert gives the wave's count and each lane's rank
// among the wave's pairs of the same expert; wave bases and expert offsets
// are exclusive prefix sums of those counts. Ids outside [0, E) are clamped
// so every pair lands in exactly one group (memory-safe on bad input).
template <typename IdT>
__global__ __launch_bounds__(1024) void moe_align_kernel(
    int* __restrict__ offsets,       // [E+1]
    int* __restrict__ sorted_pairs,  // [P]
    const IdT* __restrict__ topk_ids,  // [P]
    int P, int E) {
  __shared__ int wave_cnt[16][PS_MOE_MAX_EXPERTS];  // count, then base
  __shared__ int off_lds[PS_MOE_MAX_EXPERTS + 1];
  const int p = threadIdx.x;
  const int wave = p >> 6;
  const int lane = p & 63;
  int id = -1;
  if (p < P) {
    long v = (long)topk_ids[p];
    id = (int)(v < 0 ? 0 : (v >= E ? E - 1 : v));
  }
  int rank = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int e = 0; e < E; e++) {
    const unsigned long long m = __ballot(id == e);
    if (id == e) rank = __popcll(m & below);
    if (lane == 0) wave_cnt[wave][e] = __popcll(m);
  }
  __syncthreads();
  if (p < E) {
    int run = 0;
    for (int w = 0; w < 16; w++) {
      const int c = wave_cnt[w][p];
      wave_cnt[w][p] = run;
      run += c;
    }
    off_lds[p + 1] = run;  // expert total, prefix-summed below
  }
  __syncthreads();
  if (p == 0) {
    int run = 0;
    off_lds[0] = 0;
    for (int e = 0; e < E; e++) {
      run += off_lds[e + 1];
      off_lds[e + 1] = run;
    }
  }
  __syncthreads();
  if (p <= E) offsets[p] = off_lds[p];
  if (p < P) sorted_pairs[off_lds[id] + wave_cnt[wave][id] + rank] = p;
}

// GATED:  a = x[T, K=H],   w = experts_gate_up[E, 2N, K], N = I,
//         out_act[P, N] bf16 = silu(a.Wg^T) * (a.Wu^T); A row = pair/top_k.
// !GATED: a = act[P, K=I], w = experts_down[E, N, K],    N = H,
//         out_y[P, N] fp32 = a.W^T;                      A row = pair.
template <int M_TILES, bool GATED>
__global__ __launch_bounds__(256, 4) void moe_grouped_kernel(
    unsigned short* __restrict__ out_act, float* __restrict__ out_y,
    const unsigned short* __restrict__ a, const unsigned short* __restrict__ w,
    const int* __restrict__ offsets, const int* __restrict__ sorted_pairs,
    int top_k, int N, int K) {
  constexpr int MP = M_TILES * 16;  // rows per chunk
  constexpr int NB = GATED ? 2 : 1;
  const int e = blockIdx.y;
  const int row0 = offsets[e];
  const int count = offsets[e + 1] - row0;  // workgroup-uniform
  if (count <= 0) return;

  const int tid = threadIdx.x;
  const auto [wave, g, rc, nrow] = ps_skinny_lane_of();
  const int kchunks = K / 64;
  const long w_rows = (long)NB * N;
  const unsigned short* wg = w + ((long)e * w_rows + nrow) * K;
  const unsigned short* wu = wg + (long)N * K;  // GATED only

  // activation chunk [MP][64], 16-B slot XOR swizzle (slot ^= row&7);
  // double-buffered so one barrier per K-chunk suffices
  __shared__ __align__(16) unsigned short a_lds[2][MP][64];
  __shared__ int pair_lds[MP];  // pair id of each chunk row, -1 past count

  for (int c0 = 0; c0 < count; c0 += MP) {
    __syncthreads();  // previous chunk's readers of pair_lds / a_lds done
    if (tid < MP) {
      const int r = c0 + tid;
      pair_lds[tid] = r < count ? sorted_pairs[row0 + r] : -1;
    }
    __syncthreads();

    ps_f32x4 acc[NB][M_TILES];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
      for (int mt = 0; mt < M_TILES; mt++) acc[b][mt] = {0.f, 0.f, 0.f, 0.f};

    // B-frags for K-chunk 0; the next chunk's are fetched one iteration
    // ahead so two weight chunks are in flight per wave
    ps_bf16x8 bcur[NB][2], bnxt[NB][2];
    bcur[0][0] = *(const ps_bf16x8*)(wg + g * 8);
    bcur[0][1] = *(const ps_bf16x8*)(wg + 32 + g * 8);
    if (GATED) {
      bcur[NB - 1][0] = *(const ps_bf16x8*)(wu + g * 8);
      bcur[NB - 1][1] = *(const ps_bf16x8*)(wu + 32 + g * 8);
    }

    // ---- this thread's gather sources: MP*8 16-B slots over 256 threads
    constexpr int SLOTS = (MP * 8 + 255) / 256;
    const unsigned short* asrc[SLOTS];  // nullptr: zero-fill (past count)
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
      const int u = tid + s * 256;
      asrc[s] = nullptr;
      if (u < MP * 8) {
        const int pr = pair_lds[u >> 3];
        if (pr >= 0) {
          const long arow = GATED ? pr / top_k : pr;
          asrc[s] = a + arow * K + (u & 7) * 8;
        }
      }
    }

    for (int kc = 0; kc < kchunks; kc++) {
      const int buf = kc & 1;
      ps_bf16x8 av[SLOTS];
#pragma unroll
      for (int s = 0; s < SLOTS; s++) {
        av[s] = ps_bf16x8{};
        if (asrc[s] != nullptr)
          av[s] = *(const ps_bf16x8*)(asrc[s] + kc * 64);
      }
      if (kc + 1 < kchunks) {
        const int ko = (kc + 1) * 64;
        bnxt[0][0] = *(const ps_bf16x8*)(wg + ko + g * 8);
        bnxt[0][1] = *(const ps_bf16x8*)(wg + ko + 32 + g * 8);
        if (GATED) {
          bnxt[NB - 1][0] = *(const ps_bf16x8*)(wu + ko + g * 8);
          bnxt[NB - 1][1] = *(const ps_bf16x8*)(wu + ko + 32 + g * 8);
        }
      }
#pragma unroll
      for (int s = 0; s < SLOTS; s++) {
        const int u = tid + s * 256;
        if (u < MP * 8) {
          const int row = u >> 3;
          const int slot = u & 7;
          *(ps_bf16x8*)(&a_lds[buf][row][(slot ^ (row & 7)) * 8]) = av[s];
        }
      }
      __syncthreads();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mt = 0; mt < M_TILES; mt++) {
        const int row = mt * 16 + rc;
        ps_mfma_bf16x8 a0 = ps_as_mfma_bf16(
            *(const ps_bf16x8*)(&a_lds[buf][row][(g ^ (row & 7)) * 8]));
        ps_mfma_bf16x8 a1 = ps_as_mfma_bf16(
            *(const ps_bf16x8*)(&a_lds[buf][row][((4 + g) ^ (row & 7)) * 8]));
#pragma unroll
        for (int b = 0; b < NB; b++) {
          acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a0, ps_as_mfma_bf16(bcur[b][0]), acc[b][mt], 0, 0, 0);
          acc[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a1, ps_as_mfma_bf16(bcur[b][1]), acc[b][mt], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      // no trailing barrier: the next iteration writes the other buffer,
      // whose readers all passed this iteration's barrier
#pragma unroll
      for (int b = 0; b < NB; b++) {
        bcur[b][0] = bnxt[b][0];
        bcur[b][1] = bnxt[b][1];
      }
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
          const float s = gv / (1.f + __expf(-gv));
          out_act[pr * N + nrow] = ps_f32_to_bf16(s * uv);
        } else {
          out_y[pr * N + nrow] = acc[0][mt][r];
        }
      }
    }
  }
}

// out[t, h0..h0+3] = sum_k w[t,k] * y[t*top_k+k, h0..h0+3]; one thread per
// 4 columns, k ascending (fixed summation order).
__global__ __launch_bounds__(256) void moe_combine_kernel(
    unsigned short* __restrict__ out,  // [T, H] bf16
    const float* __restrict__ y,       // [T*top_k, H] fp32
    const float* __restrict__ topk_w,  // [T, top_k] fp32
    int T, int top_k, int H) {
  const int hq = H / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)T * hq) return;
  const int t = (int)(i / hq);
  const int h0 = (int)(i % hq) * 4;
  ps_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < top_k; k++) {
    const float wk = topk_w[t * top_k + k];
    const ps_f32x4 v =
        *(const ps_f32x4*)(y + ((long)t * top_k + k) * H + h0);
    acc += wk * v;
  }
  ps_bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = ps_f32_to_bf16(acc[j]);
  *(ps_bf16x4*)(out + (long)t * H + h0) = o;
}

extern "C" {

// The accept rule; ops.fused_moe_supported mirrors it.
int ps_fused_moe_supported(int T, int top_k, int E, int H, int I) {
  if (T < 1 || top_k < 1 || E < 1 || H < 64 || I < 64) return 0;
  if (E > PS_MOE_MAX_EXPERTS || top_k > E) return 0;
  if ((long)T * top_k > PS_MOE_MAX_PAIRS) return 0;
  if (H % 64 != 0 || I % 64 != 0) return 0;
  return 1;
}

// Scratch (all fully overwritten, no initialisation needed):
//   offsets int32[E+1], sorted_pairs int32[T*top_k],
//   act bf16[T*top_k, I], y fp32[T*top_k, H].
int ps_fused_moe(void* out, void* offsets, void* sorted_pairs, void* act,
                 void* y, const void* x, const void* w_gate_up,
                 const void* w_down, const void* topk_ids, int ids_i64,
                 const void* topk_w, int T, int top_k, int E, int H, int I,
                 hipStream_t stream) {
  if (!ps_fused_moe_supported(T, top_k, E, H, I)) return -1;
  const int P = T * top_k;
  if (ids_i64)
    moe_align_kernel<long><<<1, 1024, 0, stream>>>(
        (int*)offsets, (int*)sorted_pairs, (const long*)topk_ids, P, E);
  else
    moe_align_kernel<int><<<1, 1024, 0, stream>>>(
        (int*)offsets, (int*)sorted_pairs, (const int*)topk_ids, P, E);
  // an expert receives each token at most once, so count <= T
#define PS_MOE(MT, GATED, N, K, A, W)                                       \
  moe_grouped_kernel<MT, GATED><<<dim3((N) / 64, E), 256, 0, stream>>>(     \
      (unsigned short*)act, (float*)y, (const unsigned short*)(A),          \
      (const unsigned short*)(W), (const int*)offsets,                      \
      (const int*)sorted_pairs, top_k, N, K)
  if (T <= 16) {
    PS_MOE(1, true, I, H, x, w_gate_up);
    PS_MOE(1, false, H, I, act, w_down);
  } else if (T <= 32) {
    PS_MOE(2, true, I, H, x, w_gate_up);
    PS_MOE(2, false, H, I, act, w_down);
  } else {
    PS_MOE(4, true, I, H, x, w_gate_up);
    PS_MOE(4, false, H, I, act, w_down);
  }
#undef PS_MOE
  const long n4 = (long)T * (H / 4);
  moe_combine_kernel<<<dim3((unsigned)((n4 + 255) / 256)), 256, 0, stream>>>(
      (unsigned short*)out, (const float*)y, (const float*)topk_w, T, top_k,
      H);
  return 0;
}

}  // extern "C"
