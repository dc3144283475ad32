// Log-probabilities on the device: the chosen token's logprob and the top-N
// alternatives of a logits row in one launch, one workgroup of 16 waves per
// requested row.
//
// Contract (x_i the bf16 logit of the row rows[m], or of row m without rows):
//   logprob_i = x_i - x_max - ln sum_j exp(x_j - x_max)
//   lp[m]     logprob at token_ids[rows[m]].
//   top_*[m]  the N largest logits in descending order, equal logits in
//             ascending token id, as (id, logprob). Slots past V hold id -1
//             and -inf.
//   NaN       carries no mass, orders below -inf, is reported as -inf.
//   Rows with a +inf logit or with no finite logit are outside the contract
//   for values; every id written is still in [-1, V). A row index outside
//   [0, R) or a token id outside [0, V) reads nothing: the entry's lp is NaN
//   (and, for a bad row index, its ids are -1).
//   The output of a row is a function of the row, its token id and N alone.
//
// Design.
//   Keys and mass are the sampler's (sample_common.h): a 16-bit key that
//   orders as the bf16 value does, NaN at key 0; exp2((x - x_max) log2 e) in
//   fp32, converted once to 2^-40 fixed point and summed as 64-bit integers,
//   so Z has the same bits under any reduction order. ln Z is one fp32 log2
//   of Z * 2^-40, a number in [1, V].
//
//   Passes. Wave w owns the contiguous 512-token chunks [w cpw, (w + 1) cpw),
//   a lane 8 consecutive tokens of a chunk.
//     A  from HBM, 16 bytes per lane when V % 8 == 0 and the rows are 16-byte
//        aligned, element loads otherwise: the largest key; with N > 0 also
//        the 4096-bin count histogram of key >> 4 (LDS atomics, which hide
//        under the loads).
//     B  from L2 / Infinity Cache: the mass sum; with N > 0 also, per wave,
//        16 counters of the low 4 key bits inside the bin that pass A's
//        suffix scan selected.
//     C  N > 0 only: collect the candidates.
//   N == 0 (prompt logprobs, thousands of rows) is a kernel of its own: two
//   reads of the row, no histogram, 128 bytes of LDS.
//
//   Select. The target rank is n = min(N, V), counted over real tokens only
//   (the padding of the last chunk has key 0 like NaN but is never counted).
//   The block suffix scan over the 4096 bins and one thread over the 16
//   sub-bins give the threshold key t and need = n - #{key > t} >= 1.
//   Elements with key > t number n - need < 20 and are all in: they take
//   slots [0, n - need) through an LDS slot counter, in any order. Elements
//   with key == t fill slots [n - need, n) in ascending token id: the
//   per-wave sub-bin counters of pass B are already the per-wave tie counts,
//   so wave w knows how many ties precede its segment; it walks its chunks
//   with a wave prefix scan over the lanes' tie counts (skipped, by ballot,
//   for a chunk without ties) until need is met, and waves whose base is
//   already >= need do no tie work at all. Wave order x chunk order x lane
//   order x element order is id order. Each candidate is the 64-bit word
//   (key << 32) | ~id, all distinct; lane l of wave 0 ranks its word by
//   counting the larger ones and writes output slot rank.
//
//   No workspace, no global atomics, no floating-point sum whose order could
//   vary: LDS atomics add integers only.
//
// Compiler resource summary (gfx950), scratch 0 B in all four:
//   N > 0, 16-byte loads   93 VGPRs, 0 AGPRs,  94 SGPRs, 17720 B LDS
//   N > 0, element loads   80 VGPRs, 0 AGPRs, 106 SGPRs, 17720 B LDS
//   N == 0, 16-byte loads  46 VGPRs, 0 AGPRs,  42 SGPRs,   128 B LDS
//   N == 0, element loads  40 VGPRs, 0 AGPRs,  41 SGPRs,   128 B LDS
#include "ps_common.h"

// No packed-fp32 VALU ops in this file's device code.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                  \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "sample_common.h"

#define PS_LP_MAX_TOP 20

// logprob of a key, given the row's x_max and ln Z
PS_DEV float lp_value(unsigned key, float xmax, float lnz) {
  const float neg_inf = -__builtin_inff();
  return key == 0u ? neg_inf : (smp_val(key) - xmax) - lnz;
}

template <bool VEC, bool TOP>
__global__ __launch_bounds__(PS_SMP_THREADS) void logprobs_kernel(
    float* __restrict__ lp,                     // [M]
    int* __restrict__ top_ids,                  // [M, N]
    float* __restrict__ top_lp,                 // [M, N]
    const unsigned short* __restrict__ logits,  // [R, V] bf16
    const long* __restrict__ token_ids,         // [R]
    const int* __restrict__ rows,               // [M] or null
    long R, int V, int N) {
  __shared__ ps_u64 red[PS_SMP_WAVES];
  __shared__ unsigned cnt[TOP ? PS_SMP_BINS : 1];
  __shared__ unsigned sub[TOP ? PS_SMP_WAVES * 16 : 1];  // [wave][key & 15]
  __shared__ ps_u64 cand[TOP ? PS_LP_MAX_TOP : 1];
  __shared__ ps_u64 sel_resid;
  __shared__ unsigned sel_bin, sel_need, slot;

  const long m = __builtin_amdgcn_workgroup_id_x();
  const int tid = smp_tid(), lane = tid & 63, wave = tid >> 6;
  const float neg_inf = -__builtin_inff();
  const long r = rows ? (long)rows[m] : m;
  if (r < 0 || r >= R) {  // uniform: nothing of the batch is read
    if (tid == 0) lp[m] = __builtin_nanf("");
    if (TOP && tid < N) {
      top_ids[m * N + tid] = -1;
      top_lp[m * N + tid] = neg_inf;
    }
    return;
  }
  const unsigned short* row = logits + r * (long)V;
  const int nchunks = (V - 1) / PS_SMP_CHUNK + 1;
  const int cpw = (nchunks + PS_SMP_WAVES - 1) / PS_SMP_WAVES;
  const int c0 = wave * cpw < nchunks ? wave * cpw : nchunks;
  const int c1 = c0 + cpw < nchunks ? c0 + cpw : nchunks;
  unsigned k[8];

  if (TOP) {
    for (int b = tid; b < PS_SMP_BINS; b += PS_SMP_THREADS) cnt[b] = 0u;
    if (tid < PS_SMP_WAVES * 16) sub[tid] = 0u;
    if (tid == 0) {
      sel_bin = 0u;
      sel_resid = 1ull;
      slot = 0u;
    }
    smp_sync();
  }

  // ---- pass A, from HBM: the largest key, and the first-level counts -----
  unsigned bk = 0u;
#pragma unroll 4
  for (int c = c0; c < c1; c++) {
    const long i = (long)c * PS_SMP_CHUNK + lane * 8;
    smp_load8<VEC>(row, i, V, k);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      bk = k[j] > bk ? k[j] : bk;
      if (TOP && i + j < V) smp_lds_add(&cnt[k[j] >> 4], 1u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = smp_get(bk, lane ^ off);
    bk = o > bk ? o : bk;
  }
  if (lane == 0) red[wave] = bk;
  smp_sync();
#pragma unroll
  for (int w = 0; w < PS_SMP_WAVES; w++)
    bk = (unsigned)red[w] > bk ? (unsigned)red[w] : bk;
  smp_sync();
  const float xmax = smp_val(bk);

  // ---- the first-level bin of the n-th largest token ---------------------
  const unsigned n = N < V ? (unsigned)N : (unsigned)V;
  unsigned bin = 0u, resid = 1u;
  if (TOP) {
    unsigned total;
    const unsigned above = smp_above<unsigned>(cnt, red, total);
    smp_cross<unsigned>(cnt, above, n, &sel_bin, &sel_resid);
    smp_sync();
    bin = sel_bin;
    resid = (unsigned)sel_resid;
  }

  // ---- pass B, from cache: the mass, and the bin's per-wave sub-counts ---
  ps_u64 z = 0ull;
  for (int c = c0; c < c1; c++) {
    const long i = (long)c * PS_SMP_CHUNK + lane * 8;
    smp_load8<VEC>(row, i, V, k);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      z += smp_mass(k[j], 1u, xmax, 1.44269504088896341f);
      if (TOP && (k[j] >> 4) == bin && i + j < V)
        smp_lds_add(&sub[wave * 16 + (k[j] & 15u)], 1u);
    }
  }
  z = smp_wave_sum<ps_u64>(z);
  if (lane == 0) red[wave] = z;
  smp_sync();
  z = 0ull;
#pragma unroll
  for (int w = 0; w < PS_SMP_WAVES; w++) z += red[w];
  // Z * 2^-40 is in [1, V] for a row inside the contract
  const float lnz =
      __builtin_log2f((float)z * 9.094947017729282e-13f) * 0.693147180559945f;

  if (tid == 0) {
    const long tok = token_ids[r];
    lp[m] = (tok >= 0 && tok < V) ? lp_value(smp_key(row[tok]), xmax, lnz)
                                  : __builtin_nanf("");
  }
  if (!TOP) return;

  // ---- the threshold key t and the number of its ties to take -----------
  if (tid == 0) {
    unsigned above = 0u, q = 0u, need = 1u;
    for (int b = 15; b >= 0; b--) {
      unsigned h = 0u;
      for (int w = 0; w < PS_SMP_WAVES; w++) h += sub[w * 16 + b];
      if (above < resid && resid - above <= h) {
        q = (unsigned)b;
        need = resid - above;
      }
      above += h;
    }
    sel_bin = (bin << 4) | q;
    sel_need = need;
  }
  smp_sync();
  const unsigned t = sel_bin;
  const unsigned need = sel_need;
  const unsigned first_tie = n - need;  // = #{key > t}
  unsigned run = 0u;  // ties of key t before this wave's segment
  for (int w = 0; w < PS_SMP_WAVES; w++)
    run += w < wave ? sub[w * 16 + (t & 15u)] : 0u;

  // ---- pass C, from cache: the candidates -------------------------------
  for (int c = c0; c < c1; c++) {
    const long i = (long)c * PS_SMP_CHUNK + lane * 8;
    smp_load8<VEC>(row, i, V, k);
    unsigned ties = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const bool real = i + j < V;
      if (real && k[j] > t) {
        const unsigned s = __hip_atomic_fetch_add(
            &slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (s < first_tie)
          cand[s] = ((ps_u64)k[j] << 32) | (0xffffffffu - (unsigned)(i + j));
      }
      ties += (real && k[j] == t) ? 1u : 0u;
    }
    // wave-uniform from here: run and the ballot are the same in every lane
    if (run >= need || __builtin_amdgcn_ballot_w64(ties != 0u) == 0ull)
      continue;
    unsigned inc = ties;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned o = smp_get(inc, (lane - off) & 63);
      if (lane >= off) inc += o;
    }
    unsigned pos = run + inc - ties;  // rank among the ties of this lane's first
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (i + j < V && k[j] == t) {
        if (pos < need)
          cand[first_tie + pos] =
              ((ps_u64)t << 32) | (0xffffffffu - (unsigned)(i + j));
        pos++;
      }
    run += smp_get(inc, 63);
  }
  smp_sync();

  // ---- order the n candidates by (key desc, id asc) and write -----------
  if (wave != 0 || lane >= N) return;
  int* ids = top_ids + m * N;
  float* vals = top_lp + m * N;
  if ((unsigned)lane >= n) {  // N > V: past the row's tokens
    ids[lane] = -1;
    vals[lane] = neg_inf;
    return;
  }
  const ps_u64 mine = cand[lane];
  unsigned rank = 0u;
  for (unsigned j = 0; j < n; j++) rank += cand[j] > mine ? 1u : 0u;
  ids[rank] = (int)(0xffffffffu - (unsigned)mine);
  vals[rank] = lp_value((unsigned)(mine >> 32), xmax, lnz);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

template <bool VEC, bool TOP>
static void ps_logprobs_launch(void* lp, void* top_ids, void* top_lp,
                               const void* logits, const void* token_ids,
                               const void* rows, long M, long R, int V, int N,
                               hipStream_t stream) {
  logprobs_kernel<VEC, TOP><<<dim3((unsigned)M), PS_SMP_THREADS, 0, stream>>>(
      (float*)lp, (int*)top_ids, (float*)top_lp,
      (const unsigned short*)logits, (const long*)token_ids, (const int*)rows,
      R, V, N);
}

extern "C" int ps_logprobs(void* lp, void* top_ids, void* top_lp,
                           const void* logits, const void* token_ids,
                           const void* rows, long M, long R, int V, int N,
                           hipStream_t stream) {
  if (M < 1 || M > 0x7fffffffL || R < 1 || V < 1 || N < 0 ||
      N > PS_LP_MAX_TOP)
    return -1;
  const bool vec = V % 8 == 0 && ((unsigned long)logits & 15ul) == 0;
  auto fn = N > 0 ? (vec ? ps_logprobs_launch<true, true>
                         : ps_logprobs_launch<false, true>)
                  : (vec ? ps_logprobs_launch<true, false>
                         : ps_logprobs_launch<false, false>);
  fn(lp, top_ids, top_lp, logits, token_ids, rows, M, R, V, N, stream);
  return 0;
}
