// Stochastic sampling on the device: temperature, top-k, min-p, top-p and the
// draw in one kernel, one workgroup of 16 waves per logits row.
//
// Contract (x_i the bf16 logit, T the temperature, s_i = x_i / T):
//   T == 0   argmax, smallest index among ties (what greedy_sample_kernel
//            gives), so a mixed batch is one launch.
//   top-k    (0 < k < V) keep x_i >= the k-th largest value; ties all stay.
//   min-p    (min_p > 0) keep s_i - s_max >= ln(min_p).
//   top-p    (top_p < 1) over the survivors, sorted descending, b is the last
//            token whose preceding mass is < top_p of the total; keep every
//            survivor with p_i >= p_b, the whole tie class of b included.
//   draw     the first kept token, in ascending token id, whose running sum
//            of p_i exceeds u * Z_kept.
//
// Design.
//   Keys. A bf16 logit has 65536 values, and x / T is monotone in x, so the
//   bits are mapped to a 16-bit key that sorts as the value does (-0 folded
//   into +0, NaN and the padding of the last chunk to key 0, below -inf).
//   Each filter is then a key threshold and the kept set is
//   key >= max(thresholds): nothing is sorted.
//
//   Mass. p_i = exp2((x_i - x_max) * log2(e) / T) in fp32, in (0, 1], is
//   converted once to 40-bit fixed point (1.0 = 2^40) and every sum after
//   that is a 64-bit integer sum: histogram bins, wave and block reductions,
//   the running sum of the draw. Integer addition commutes, so LDS atomics
//   and any reduction order give the same bits, the output is a function of
//   (logits, params, u) alone, and the draw's walk cannot run off the end
//   (floor(u * Z) < Z in integers). V * 2^40 < 2^63 for every int32 V, and
//   a token 2^-40 of the largest one weighs nothing.
//
//   Thresholds by radix select, 12 + 4 bits. A pass over the row adds each
//   element to one of 4096 LDS bins (key >> 4): 4096 rather than 256 bins so
//   that a wave's 64 atomics spread over mantissa bits and do not pile onto
//   the two or three exponents a row lives in. A block-wide suffix scan over
//   the bins (thread t owns the four bins 4 * (1023 - t) ..) finds the bin in
//   which the running count reaches k, or the running mass reaches
//   top_p * Z; a second pass histograms the low 4 bits of that bin's
//   elements and one thread finishes the select. top-k selects on counts
//   (u32 bins), top-p on mass (u64 bins) over the top-k and min-p survivors;
//   the min-p threshold is arithmetic on x_max. Passes a row does not need
//   are skipped: with no filter a row is read for the max, for the segment
//   masses, and by one wave for the walk.
//
//   Draw. Wave w owns the contiguous chunks [w * cpw, (w + 1) * cpw) of 512
//   tokens, a lane 8 consecutive tokens of a chunk, so wave order, lane order
//   and element order are token-id order. The 16 segment masses are scanned;
//   only the wave whose segment holds floor(u * Z) walks it, a chunk at a
//   time with a wave prefix scan in the chunk where the sum crosses.
//
//   Memory. A row (250 KB at V = 128256) does not fit in LDS. The max pass
//   streams it from HBM once, 16 bytes per lane when rows are 16-byte
//   aligned (V % 8 == 0), element loads otherwise; later passes re-read it
//   from L2 / Infinity Cache. No workspace, no global atomics.
//
//   Uniform. Philox-4x32-10, counter {ctr lo, ctr hi, 0, 0}, key {key lo,
//   key hi}; u = (word0 >> 8) * 2^-24. u_in, where given, replaces it.
//
// Compiler resource summary (gfx950): 60 VGPRs for the 16-byte-load form and
// 80 for the element-load form, 0 AGPRs, 56 SGPRs, 32912 B LDS, 0 B scratch.
#include "ps_common.h"

// No packed-fp32 VALU ops in this file's device code.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                  \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// keys, 8-token loads, fixed-point mass, scans: shared with logprobs.hip
#include "sample_common.h"

struct ps_sample_rec {  // 32 bytes, one per row
  float temperature;
  int top_k;
  float top_p;
  float min_p;
  ps_u64 key;
  ps_u64 counter;
};

// smallest key whose value is >= f
PS_DEV unsigned smp_key_ceil(float f) {
  const unsigned bits = __builtin_bit_cast(unsigned, f);
  // toward +inf: truncation for a negative value, round-up for a positive one
  const unsigned b16 =
      (bits & 0x80000000u) ? (bits >> 16) : ((bits + 0xffffu) >> 16);
  return smp_key((unsigned short)b16);
}

// smp_cross over the 16 second-level bins, by one thread
template <typename T>
PS_DEV unsigned smp_cross16(const T* hist, T target) {
  T above = 0;
  unsigned q = 0;
  for (int b = 15; b >= 0; b--) {
    const T h = hist[b];
    if (above < target && target - above <= h) q = (unsigned)b;
    above += h;
  }
  return q;
}

PS_DEV float smp_philox_uniform(ps_u64 key, ps_u64 counter) {
  unsigned c0 = (unsigned)counter, c1 = (unsigned)(counter >> 32);
  unsigned c2 = 0u, c3 = 0u;
  unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
  for (int r = 0; r < 10; r++) {
    const ps_u64 p0 = (ps_u64)0xD2511F53u * c0, p1 = (ps_u64)0xCD9E8D57u * c2;
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
    const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * 5.9604644775390625e-8f;  // 2^-24
}

template <bool VEC>
__global__ __launch_bounds__(PS_SMP_THREADS) void sample_kernel(
    long* __restrict__ out,                     // [R]
    float* __restrict__ u_out,                  // [R] or null
    const unsigned short* __restrict__ logits,  // [R, V] bf16
    const ps_sample_rec* __restrict__ params,   // [R]
    const float* __restrict__ u_in,             // [R] or null
    int V) {
  __shared__ ps_u64 hist[PS_SMP_BINS];  // u32 counts use the front half
  __shared__ ps_u64 red[PS_SMP_WAVES];
  __shared__ ps_u64 sel_resid;
  __shared__ unsigned sel_bin;
  unsigned* cnt = (unsigned*)hist;

  const long r = __builtin_amdgcn_workgroup_id_x();
  const unsigned short* row = logits + r * (long)V;
  const ps_sample_rec rec = params[r];
  const int tid = smp_tid(), lane = tid & 63, wave = tid >> 6;
  const int nchunks = (V - 1) / PS_SMP_CHUNK + 1;
  const int cpw = (nchunks + PS_SMP_WAVES - 1) / PS_SMP_WAVES;
  const int c0 = wave * cpw < nchunks ? wave * cpw : nchunks;
  const int c1 = c0 + cpw < nchunks ? c0 + cpw : nchunks;
  unsigned k[8];

  float u = u_in ? u_in[r] : smp_philox_uniform(rec.key, rec.counter);
  u = __builtin_fminf(__builtin_fmaxf(u, 0.0f), 0.99999994f);
  if (u_out && tid == 0) u_out[r] = u;

  // ---- pass 1, from HBM: the largest key and its first position ----------
  unsigned bk = 0u, bi = 0u;
#pragma unroll 4
  for (int c = c0; c < c1; c++) {
    const long i = (long)c * PS_SMP_CHUNK + lane * 8;
    smp_load8<VEC>(row, i, V, k);
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (k[j] > bk) {  // ascending positions: the first of equals stays
        bk = k[j];
        bi = (unsigned)i + j;
      }
  }
  ps_u64 best = ((ps_u64)bk << 32) | (0xffffffffu - bi);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const ps_u64 o = smp_get(best, lane ^ off);
    best = o > best ? o : best;
  }
  if (lane == 0) red[wave] = best;
  smp_sync();
#pragma unroll
  for (int w = 0; w < PS_SMP_WAVES; w++) best = red[w] > best ? red[w] : best;
  smp_sync();
  const unsigned kmax = (unsigned)(best >> 32);
  const long amax = (long)(0xffffffffu - (unsigned)best);
  // the draw overwrites this; a row with no mass to draw from (all NaN,
  // +inf logits) keeps the argmax
  if (tid == 0) out[r] = amax;
  if (rec.temperature == 0.0f) return;

  const float xmax = smp_val(kmax);
  const float c = 1.44269504088896341f / rec.temperature;
  unsigned thr = 1u;  // key 0 is NaN and padding: never kept

  // ---- top-k: the k-th largest key, a radix select on counts -------------
  if (rec.top_k > 0 && rec.top_k < V) {
    for (int b = tid; b < PS_SMP_BINS; b += PS_SMP_THREADS) cnt[b] = 0u;
    if (tid == 0) sel_bin = 0u;
    smp_sync();
    for (int ch = c0; ch < c1; ch++) {
      smp_load8<VEC>(row, (long)ch * PS_SMP_CHUNK + lane * 8, V, k);
#pragma unroll
      for (int j = 0; j < 8; j++) smp_lds_add(&cnt[k[j] >> 4], 1u);
    }
    smp_sync();
    unsigned total;
    const unsigned above = smp_above<unsigned>(cnt, red, total);
    smp_cross<unsigned>(cnt, above, (unsigned)rec.top_k, &sel_bin,
                        &sel_resid);
    smp_sync();
    const unsigned bin = sel_bin;
    const unsigned resid = (unsigned)sel_resid;
    smp_sync();
    if (tid < 16) cnt[tid] = 0u;
    smp_sync();
    for (int ch = c0; ch < c1; ch++) {
      smp_load8<VEC>(row, (long)ch * PS_SMP_CHUNK + lane * 8, V, k);
#pragma unroll
      for (int j = 0; j < 8; j++)
        if ((k[j] >> 4) == bin) smp_lds_add(&cnt[k[j] & 15u], 1u);
    }
    smp_sync();
    if (tid == 0) sel_bin = (bin << 4) | smp_cross16<unsigned>(cnt, resid);
    smp_sync();
    thr = sel_bin > thr ? sel_bin : thr;
    smp_sync();
  }

  // ---- min-p: s_i - s_max >= ln(min_p), i.e. x_i >= x_max + T ln(min_p) --
  if (rec.min_p > 0.0f) {
    const unsigned t =
        smp_key_ceil(xmax + rec.temperature * __builtin_logf(rec.min_p));
    thr = t > thr ? t : thr;
  }
  thr = thr > kmax ? kmax : thr;  // the largest logit is always kept

  // ---- top-p: a radix select on mass over the survivors ------------------
  if (rec.top_p < 1.0f) {
    for (int b = tid; b < PS_SMP_BINS; b += PS_SMP_THREADS) hist[b] = 0ull;
    if (tid == 0) sel_bin = 0xffffffffu;
    smp_sync();
    for (int ch = c0; ch < c1; ch++) {
      smp_load8<VEC>(row, (long)ch * PS_SMP_CHUNK + lane * 8, V, k);
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (k[j] >= thr)
          smp_lds_add(&hist[k[j] >> 4], smp_mass(k[j], thr, xmax, c));
    }
    smp_sync();
    ps_u64 Z;
    const ps_u64 above = smp_above<ps_u64>(hist, red, Z);
    // a tie class is kept when the mass above it is < top_p * Z: the
    // smallest integer no less than top_p * Z is the select's target
    const double pz = (double)rec.top_p * (double)Z;
    ps_u64 target = (ps_u64)pz;
    if ((double)target < pz) target++;
    target = target < 1ull ? 1ull : (target > Z ? Z : target);
    smp_cross<ps_u64>(hist, above, target, &sel_bin, &sel_resid);
    smp_sync();
    const unsigned bin = sel_bin;
    const ps_u64 resid = sel_resid;
    smp_sync();
    if (bin != 0xffffffffu) {  // Z == 0 leaves the set alone
      if (tid < 16) hist[tid] = 0ull;
      smp_sync();
      for (int ch = c0; ch < c1; ch++) {
        smp_load8<VEC>(row, (long)ch * PS_SMP_CHUNK + lane * 8, V, k);
#pragma unroll
        for (int j = 0; j < 8; j++)
          if (k[j] >= thr && (k[j] >> 4) == bin)
            smp_lds_add(&hist[k[j] & 15u], smp_mass(k[j], thr, xmax, c));
      }
      smp_sync();
      if (tid == 0) sel_bin = (bin << 4) | smp_cross16<ps_u64>(hist, resid);
      smp_sync();
      thr = sel_bin > thr ? sel_bin : thr;
    }
  }

  // ---- draw, in token-id order -------------------------------------------
  ps_u64 seg = 0ull;
  for (int ch = c0; ch < c1; ch++) {
    smp_load8<VEC>(row, (long)ch * PS_SMP_CHUNK + lane * 8, V, k);
#pragma unroll
    for (int j = 0; j < 8; j++) seg += smp_mass(k[j], thr, xmax, c);
  }
  seg = smp_wave_sum<ps_u64>(seg);
  if (lane == 0) red[wave] = seg;
  smp_sync();
  ps_u64 run = 0ull, Zk = 0ull;
#pragma unroll
  for (int w = 0; w < PS_SMP_WAVES; w++) {
    const ps_u64 x = red[w];
    if (w < wave) run += x;
    Zk += x;
  }
  // floor(u * Zk) < Zk: u <= 1 - 2^-24 and the product's rounding is 2^-53
  const ps_u64 target = (ps_u64)((double)u * (double)Zk);
  if (!(run <= target && target - run < seg)) return;  // whole waves leave
  for (int ch = c0; ch < c1; ch++) {
    const long i = (long)ch * PS_SMP_CHUNK + lane * 8;
    smp_load8<VEC>(row, i, V, k);
    ps_u64 m[8], ls = 0ull;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      m[j] = smp_mass(k[j], thr, xmax, c);
      ls += m[j];
    }
    ps_u64 inc = ls;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const ps_u64 o = smp_get(inc, (lane - off) & 63);
      if (lane >= off) inc += o;
    }
    const ps_u64 tot = smp_get(inc, 63);
    if (target - run < tot) {  // the sum crosses in this chunk
      ps_u64 a = run + inc - ls;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (a <= target && target - a < m[j]) out[r] = i + j;
        a += m[j];
      }
      return;
    }
    run += tot;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" int ps_sample(void* out, void* u_out, const void* logits,
                         const void* params, const void* u_in, long R, int V,
                         hipStream_t stream) {
  if (R < 1 || R > 0x7fffffffL || V < 1) return -1;
  const bool vec = V % 8 == 0 && ((unsigned long)logits & 15ul) == 0;
  if (vec)
    sample_kernel<true><<<dim3((unsigned)R), PS_SMP_THREADS, 0, stream>>>(
        (long*)out, (float*)u_out, (const unsigned short*)logits,
        (const ps_sample_rec*)params, (const float*)u_in, V);
  else
    sample_kernel<false><<<dim3((unsigned)R), PS_SMP_THREADS, 0, stream>>>(
        (long*)out, (float*)u_out, (const unsigned short*)logits,
        (const ps_sample_rec*)params, (const float*)u_in, V);
  return 0;
}
