// Device helpers shared by the per-row vocabulary kernels, sample.hip and
// logprobs.hip: the monotone 16-bit key of a bf16 logit, the 8-token loads,
// 40-bit fixed-point mass, and the wave / block scans of the radix select.
// Include it inside the file's no-packed-fp32-ops attribute region.
#pragma once

#include "ps_common.h"

typedef unsigned long long ps_u64;

#define PS_SMP_THREADS 1024
#define PS_SMP_WAVES 16
#define PS_SMP_CHUNK 512  // tokens per wave per step: 64 lanes x 8
#define PS_SMP_BINS 4096  // first-level bins: key >> 4

// bf16 bits -> key that orders as the value does
PS_DEV unsigned smp_key(unsigned short b) {
  unsigned u = b;
  if ((u & 0x7fffu) > 0x7f80u) return 0u;  // NaN: below everything
  if (u == 0x8000u) u = 0u;                // -0 == +0
  return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}

PS_DEV float smp_val(unsigned key) {
  const unsigned u = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return ps_bf16_to_f32((unsigned short)u);
}

// p_i in fixed point; 0 for a token outside the kept set
PS_DEV ps_u64 smp_mass(unsigned key, unsigned thr, float xmax, float c) {
  float e = __builtin_amdgcn_exp2f((smp_val(key) - xmax) * c);
  e = __builtin_fmaxf(e, 0.0f);  // inf - inf
  const float a = e * 65536.0f;
  const unsigned hi = (unsigned)a;
  const unsigned lo = (unsigned)((a - (float)hi) * 16777216.0f);
  const ps_u64 m = ((ps_u64)hi << 24) + lo;
  return key >= thr ? m : 0ull;
}

// keys of the 8 tokens from i on; tokens past the row's end get key 0
template <bool VEC>
PS_DEV void smp_load8(const unsigned short* __restrict__ row, long i, int V,
                      unsigned (&k)[8]) {
  if (VEC) {
    ps_bf16x8 v = {0xffff, 0xffff, 0xffff, 0xffff,
                   0xffff, 0xffff, 0xffff, 0xffff};
    if (i < V) v = *(const ps_bf16x8*)(row + i);  // V % 8 == 0: all or none
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = smp_key(v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++)
      k[j] = (i + j < V) ? smp_key(row[i + j]) : 0u;
  }
}

// Under the including file's target attribute the HIP header's inline
// wrappers (__syncthreads, __shfl*, atomicAdd, ...) would stay out of line,
// so the kernels are written with the builtins beneath them.
PS_DEV void smp_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

PS_DEV int smp_tid() { return (int)__builtin_amdgcn_workitem_id_x(); }
PS_DEV int smp_lane() { return smp_tid() & 63; }

// v of lane src (0..63)
PS_DEV unsigned smp_get(unsigned v, int src) {
  return (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)v);
}
PS_DEV ps_u64 smp_get(ps_u64 v, int src) {
  const unsigned lo = smp_get((unsigned)v, src);
  const unsigned hi = smp_get((unsigned)(v >> 32), src);
  return ((ps_u64)hi << 32) | lo;
}

// LDS integer add, no return value used: commutative, so order-free
template <typename T>
PS_DEV void smp_lds_add(T* p, T v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <typename T>
PS_DEV T smp_wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += smp_get(v, smp_lane() ^ off);
  return v;
}

// Exclusive prefix of v in thread order and the block total. red holds 16.
template <typename T>
PS_DEV T smp_block_scan(T v, ps_u64* red, T& total) {
  const int lane = smp_lane();
  const int wave = smp_tid() >> 6;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = smp_get(inc, (lane - off) & 63);
    if (lane >= off) inc += o;
  }
  if (lane == 63) red[wave] = inc;
  smp_sync();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < PS_SMP_WAVES; w++) {
    const T x = (T)red[w];
    if (w < wave) base += x;
    tot += x;
  }
  smp_sync();
  total = tot;
  return base + inc - v;
}

// Thread t owns bins 4 * (1023 - t) .. + 3, so thread order is descending
// bin order: the sum of the bins above this thread's, and the total.
template <typename T>
PS_DEV T smp_above(const T* hist, ps_u64* red, T& total) {
  const int b = 4 * (PS_SMP_THREADS - 1 - smp_tid());
  return smp_block_scan<T>(hist[b] + hist[b + 1] + hist[b + 2] + hist[b + 3],
                           red, total);
}

// The bin in which the descending running sum reaches target
// (above < target <= above + bin), and target - above there. One thread
// finds it when 0 < target <= total.
template <typename T>
PS_DEV void smp_cross(const T* hist, T above, T target, unsigned* bin,
                      ps_u64* resid) {
  const int b = 4 * (PS_SMP_THREADS - 1 - smp_tid());
#pragma unroll
  for (int q = 3; q >= 0; q--) {
    const T h = hist[b + q];
    if (above < target && target - above <= h) {
      *bin = (unsigned)(b + q);
      *resid = (ps_u64)(target - above);
    }
    above += h;
  }
}
