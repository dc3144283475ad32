// What the fused MoE expert kernels (moe_fused.hip, moe_fused_w4.hip) share:
// the pair/expert bounds and moe_align, the device-side counting sort of the
// routed (token, k) pairs by expert.
#pragma once

#include "skinny_common.h"

#define PS_MOE_MAX_PAIRS 1024
#define PS_MOE_MAX_EXPERTS 64

// One workgroup of 1024 threads, thread p owns pair p = t*top_k + k.
// Per wave, a ballot per expert gives the wave's count and each lane's rank
// among the wave's pairs of the same expert; wave bases and expert offsets
// are exclusive prefix sums of those counts. Ids outside [0, E) are clamped
// so every pair lands in exactly one group (memory-safe on bad input).
// static: a file that launches it has its own copy, like every other kernel
// of that file.
template <typename IdT>
static __global__ __launch_bounds__(1024) void moe_align_kernel(
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

static inline void ps_launch_moe_align(void* offsets, void* sorted_pairs,
                                       const void* topk_ids, int ids_i64,
                                       int P, int E, hipStream_t stream) {
  if (ids_i64)
    moe_align_kernel<long><<<1, 1024, 0, stream>>>(
        (int*)offsets, (int*)sorted_pairs, (const long*)topk_ids, P, E);
  else
    moe_align_kernel<int><<<1, 1024, 0, stream>>>(
        (int*)offsets, (int*)sorted_pairs, (const int*)topk_ids, P, E);
}
