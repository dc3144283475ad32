// MFMA chunked-prefill attention for head_dim 64 on gfx950 (Llama-3.2-1B
// class models; bf16 or fp8 e4m3 paged KV). Reached as variant 5 of
// paged_attn_prefill_mfma when head_dim == 64.
//
// The tile/work split is the one of csrc/prefill_mfma32.hip (v5), so the
// engine's tiles, the split rule and the numeric contract carry over:
//   grid = (work items, kv splits), block = 512 (8 waves). The 8 waves are
//   GQW head columns x (8/GQW) groups of 32 q rows; all GQW heads of a kv
//   head share one K/V staging pass. KV is consumed in 64-key chunks.
//
// What differs, and why. At D = 64 a wave does 8 + 8 MFMAs per chunk
// instead of 16 + 16, while the softmax (64 keys x 32 rows) and v5's round
// trip of P through 32 KiB of LDS cost what they did: the kernel would be
// softmax- and LDS-bound. So here:
//   * QK^T is swapped as in v5: S^T[kv, q] = mfma_32x32x16(K_frag, Q_frag).
//     A lane owns ONE q column; row max and sum are lane-local plus one
//     shfl_xor(., 32).
//   * PV is swapped too: O^T[d, q] = mfma_32x32x16(V^T_frag, P^T_frag).
//     A lane's S^T accumulators hold kv rows (r&3) + 8*(r>>2) + 4*hi of the
//     32-key tile (layout verified by csrc/tools/mfma32_probe.hip), so
//     registers 8j..8j+7 of both half-waves together are keys [16j, 16j+16)
//     exactly once, in the k order 4*hi + (i&3) + 8*(i>>2) (the probe's
//     k-pattern 1). Packed to bf16 they ARE the B operand of k-step j. The
//     V^T A-fragment supplies the same permutation because V^T is stored in
//     LDS with bits 2 and 3 of the key index swapped inside every 16 keys:
//     one 16-byte LDS read per fragment. P never touches LDS, there is no P
//     barrier, and the O rescale factor is the lane's own scalar (v5 needs
//     16 shuffles per rescale).
//   * O^T is 2 x 16 fp32 registers; with no p_lds the K and V^T tiles
//     (8 KiB each per chunk) are double-buffered in 32 KiB of LDS: ONE
//     barrier per chunk instead of two. Chunk c+1 is written to the other
//     buffer before chunk c's MFMAs and chunk c+2's global loads are issued
//     under them.
//   * P is packed with the hardware bf16 conversion (round to nearest even,
//     as ps_f32_to_bf16) and exp2 is the raw v_exp_f32.
//   * Epilogue: a lane holds 4 consecutive d per register quad. The two
//     half-waves swap one quad each (shfl_xor 32), so every lane stores
//     16-byte row segments; split partials are stored as float4. No LDS.
//   * A combine kernel of its own: 16 lanes x float4 per (token, head).
//
// Numeric contract (tests/attention_criteria.py "mfma", wave_rows = 32):
// q * (scale * log2 e) rounded to bf16 once; fp32 scores and accumulators in
// the exp2 domain; online softmax in 64-key chunks; defer-max with
// PS_RESCALE_THR32 over the wave's 32 rows; P rounded to bf16 before PV, row
// sum from the unrounded P.
//
// Compiler summary (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage):
//   kernel, GQW 1/2/4     VGPRs        AGPRs  scratch  LDS      waves/SIMD
//   bf16 KV               158/160/160  0      0        32768 B  3
//   fp8 KV                162/164/164  0      0        32768 B  3
//   combine               25           0      0        0        8
// An 8-wave workgroup needs 2 waves/SIMD, so one workgroup is resident per
// CU (as for v5). Capped at 128 VGPRs (two workgroups per CU) the compiler
// spills 32-41 registers, so the cap is not set; see TODO.md.
#include "ps_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 ps_mbf16x8;
typedef __attribute__((ext_vector_type(16))) float ps_mf32x16;
typedef __attribute__((ext_vector_type(8))) float ps_mf32x8;
typedef __attribute__((ext_vector_type(4))) unsigned int ps_u32x4;

PS_DEV ps_mbf16x8 ps_as_mbf16_64(ps_bf16x8 u) {
  union {
    ps_bf16x8 u16;
    ps_mbf16x8 bf;
  } v;
  v.u16 = u;
  return v.bf;
}

#define PS_CHUNK64 64  // KV tokens per softmax step and per LDS buffer

// tile_info: int4 per tile = (seq_row, q_token_start, q_pos_start, n_rows),
// n_rows <= 32 * (8 / GQW). Split-KV (gridDim.y > 1): split s takes chunks
// s, s+S, ... and writes unnormalised (o, m, l) to the workspace.
template <int GQW, typename KVT>
__global__ __launch_bounds__(512, 2) void paged_attn_prefill_mfma64_kernel(
    unsigned short* __restrict__ out,            // [T, QH, 64]
    float* __restrict__ ws_o,    // [S, T, QH, 64] (splits > 1)
    float* __restrict__ ws_ml,   // [2, S, T, QH]
    long q_tokens,
    const unsigned short* __restrict__ q,        // [T, QH, 64], rows strided
    const KVT* __restrict__ k_cache,             // [NB, KH, 16, 64]
    const KVT* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [S, max_blocks]
    const int* __restrict__ tile_info,     // [NT, 4]
    int max_blocks, float scale, int KH, int GQ, long q_stride,
    int QH, int n_work, int window) {
  const int split = blockIdx.y;
  const int n_splits = gridDim.y;
  using KVTr = ps_kv_traits<KVT>;
  using kvec8 = typename KVTr::vec8;
  using kvec4 = typename KVTr::vec4;
  constexpr int D = 64;
  constexpr int BS = 16;        // page size in tokens
  constexpr int NKS = D / 16;   // QK k-steps over head dim (4)
  constexpr int ROWH = 8 / GQW; // 32-row groups per tile

  // XCD swizzle as in v5: contiguous work chunks per XCD
  const int W = n_work;  // n_tiles * KH * (GQ/GQW)
  const int cpx = (W + 7) >> 3;
  const int w = (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
  if (w >= W) return;
  const int n_grp = GQ / GQW;
  const int n_tiles = W / (n_grp * KH);
  const int tile = w % n_tiles;
  const int g_grp = (w / n_tiles) % n_grp;
  const int kvh = w / (n_tiles * n_grp);
  const int seq_row = tile_info[tile * 4 + 0];
  const int q_tok0 = tile_info[tile * 4 + 1];
  const int q_pos0 = tile_info[tile * 4 + 2];
  const int n_rows = tile_info[tile * 4 + 3];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;   // half-wave
  const int rc = lane & 31;   // q row (B/D col), or kv / d row (A row)
  const int qh = kvh * GQ + g_grp * GQW + (wave / ROWH);
  const int wq0 = (wave % ROWH) * 32;  // wave's first local q row

  const int* bt = block_tables + (long)seq_row * max_blocks;
  const int ctx_limit = q_pos0 + n_rows;
  const int n_pages = (ctx_limit + BS - 1) / BS;
  const int n_chunks = (ctx_limit + PS_CHUNK64 - 1) / PS_CHUNK64;

  // k_lds[buf][key][d]: 16-byte slot XOR-swizzled by key & 7.
  // v_t[buf][d][key']: key' = key with bits 2 and 3 swapped inside each 16
  // (the PV k order, see the header); octet XOR-swizzled by d & 7.
  __shared__ __align__(16) unsigned short k_lds[2][PS_CHUNK64][D];
  __shared__ __align__(16) unsigned short v_t[2][D][PS_CHUNK64];

  // ---- Q fragments: B operand, lane supplies Q[q=rc][d=ks*16+hi*8+i] ----
  const int q_row_clamped = min(wq0 + rc, n_rows - 1);
  const unsigned short* qrow =
      q + (long)(q_tok0 + q_row_clamped) * q_stride + (long)qh * D;
  const float qmul = scale * 1.44269504f;  // exp2-domain softmax
  ps_mbf16x8 q_frag[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ks++) {
    ps_bf16x8 qv = *(const ps_bf16x8*)(qrow + ks * 16 + hi * 8);
    ps_bf16x8 qs;
#pragma unroll
    for (int j = 0; j < 8; j++)
      qs[j] = ps_f32_to_bf16(ps_bf16_to_f32(qv[j]) * qmul);
    q_frag[ks] = ps_as_mbf16_64(qs);
  }

  // online-softmax state of q row rc: lane-local scalars
  float m_run = PS_NEG_INF, l_run = 0.f;
  ps_mf32x16 o_acc[2];  // lane holds O^T[d = dt*32 + roff(r, hi)][q = rc]
#pragma unroll
  for (int dt = 0; dt < 2; dt++)
#pragma unroll
    for (int r = 0; r < 16; r++) o_acc[dt][r] = 0.f;

  const int q_pos = q_pos0 + wq0 + rc;  // this lane's q position
  const int wave_pos_max = q_pos0 + min(wq0 + 31, n_rows - 1);
  const int wave_win_lo =
      window > 0 ? max(0, (q_pos0 + wq0) - window + 1) : 0;

  // ---- staging assignments (512 threads, 64 keys x 64 dims each of K, V)
  // K: one 8-dim segment per thread: key t>>3, slot t&7.
  // V: a key pair x 4 dims per thread, register-transposed: pair t&31,
  //    dim slice t>>5. A pair never straddles a page.
  const int ktok = tid >> 3, kslot = tid & 7;
  const int vtk = (tid & 31) * 2, vds = tid >> 5;
  const int vu = vtk & 15;
  const int vpos = (vu & 3) | ((vu & 4) << 1) | ((vu & 8) >> 1);
  const int voct = (vtk >> 4) * 2 + (vpos >> 3);
  // table padding is never dereferenced: the page index is clamped to the
  // tile's last page, whose slots past the context hold finite values
  auto k_seg_ptr = [&](int chunk) {
    const int tok = chunk * PS_CHUNK64 + ktok;
    const long pg = bt[min(tok / BS, n_pages - 1)];
    return k_cache + ((pg * KH + kvh) * BS + (tok & (BS - 1))) * D +
           kslot * 8;
  };
  auto v_pair_ptr = [&](int chunk) {
    const int tok = chunk * PS_CHUNK64 + vtk;
    const long pg = bt[min(tok / BS, n_pages - 1)];
    return v_cache + ((pg * KH + kvh) * BS + (tok & (BS - 1))) * D + vds * 4;
  };
  kvec8 kstage;
  kvec4 vstage[2];
  auto load_stage = [&](int chunk) {
    const KVT* vq = v_pair_ptr(chunk);
    kstage = *(const kvec8*)k_seg_ptr(chunk);
    vstage[0] = *(const kvec4*)vq;
    vstage[1] = *(const kvec4*)(vq + D);
  };
  auto write_stage = [&](int b) {
    *(ps_bf16x8*)(&k_lds[b][ktok][(kslot ^ (ktok & 7)) * 8]) =
        KVTr::to_bf16x8(kstage);
#pragma unroll
    for (int dd = 0; dd < 4; dd++) {
      const int d = vds * 4 + dd;
      const unsigned int pair =
          (unsigned int)KVTr::to_bf16(vstage[0][dd]) |
          ((unsigned int)KVTr::to_bf16(vstage[1][dd]) << 16);
      *(unsigned int*)(&v_t[b][d][((voct ^ (d & 7)) * 8) + (vpos & 7)]) =
          pair;
    }
  };

  // prologue: chunk `split` into buffer 0, the one after it into registers
  if (split < n_chunks) {
    load_stage(split);
    write_stage(0);
    if (split + n_splits < n_chunks) load_stage(split + n_splits);
  }
  __syncthreads();

  int buf = 0;
  for (int chunk = split; chunk < n_chunks; chunk += n_splits, buf ^= 1) {
    const int tok0 = chunk * PS_CHUNK64;
    // the other buffer was last read before the barrier that ended the
    // previous iteration; what is written here is read after this one's
    if (chunk + n_splits < n_chunks) {
      write_stage(buf ^ 1);
      if (chunk + 2 * n_splits < n_chunks)
        load_stage(chunk + 2 * n_splits);  // lands under this chunk's MFMAs
    }

    const bool wave_active = (wq0 < n_rows) && (tok0 <= wave_pos_max) &&
                             (tok0 + PS_CHUNK64 > wave_win_lo);
    if (wave_active) {
      // ---- swapped QK^T: S^T[kv = kt*32 + .., q] over 2 key tiles ----
      ps_mf32x16 s_frag[2];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kt = 0; kt < 2; kt++) {
#pragma unroll
        for (int r = 0; r < 16; r++) s_frag[kt][r] = 0.f;
        const int krow = kt * 32 + rc;  // A row: key in the chunk
#pragma unroll
        for (int ks = 0; ks < NKS; ks++) {
          const int slot = (ks * 2 + hi) ^ (krow & 7);
          ps_mbf16x8 k_frag = ps_as_mbf16_64(
              *(const ps_bf16x8*)(&k_lds[buf][krow][slot * 8]));
          s_frag[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              k_frag, q_frag[ks], s_frag[kt], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      // ---- mask + lane-local online softmax ----
      bool full_chunk = (tok0 + PS_CHUNK64 - 1 <= q_pos0 + wq0) &&
                        (wq0 + 31 < n_rows);
      if (window > 0)
        full_chunk = full_chunk && (tok0 >= wave_pos_max - window + 1);
      float m_new = m_run;
      if (!full_chunk) {
        const bool row_real = (wq0 + rc) < n_rows;
#pragma unroll
        for (int kt = 0; kt < 2; kt++) {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int kv_pos =
                tok0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            bool valid = row_real && (kv_pos <= q_pos);
            if (window > 0) valid = valid && (kv_pos > q_pos - window);
            s_frag[kt][r] = valid ? s_frag[kt][r] : PS_NEG_INF;
          }
        }
      }
#pragma unroll
      for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int r = 0; r < 16; r++) m_new = fmaxf(m_new, s_frag[kt][r]);
      m_new = fmaxf(m_new, __shfl_xor(m_new, 32));  // join half-waves
      // defer-max: skip the rescale while no row's max grew by the threshold
      constexpr float PS_RESCALE_THR32 = 11.54f;  // 8 nats in log2 units
      const bool grew = (m_new > m_run + PS_RESCALE_THR32) ||
                        (m_run == PS_NEG_INF && m_new > PS_NEG_INF);
      if (__any(grew)) {
        const float corr = exp2f(m_run - m_new);  // this lane's own q row
        l_run *= corr;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 2; dt++)
#pragma unroll
          for (int r = 0; r < 16; r++) o_acc[dt][r] *= corr;
      }
      // a row that has met no key keeps m_run = PS_NEG_INF: its P is 0
      const bool row_seen = m_run > PS_NEG_INF;
      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; kt++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float e = __builtin_amdgcn_exp2f(s_frag[kt][r] - m_run);
          const float p = row_seen ? e : 0.f;
          s_frag[kt][r] = p;
          psum += p;
        }
      }
      l_run += psum + __shfl_xor(psum, 32);
      // ---- swapped PV: O^T[d, q] += V^T[d, kv] P^T[kv, q]; registers
      // 8j..8j+7 of the S^T tile are the B operand of k-step j ----
#pragma unroll
      for (int kt = 0; kt < 2; kt++) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
          ps_mf32x8 pf;
#pragma unroll
          for (int i = 0; i < 8; i++) pf[i] = s_frag[kt][8 * j + i];
          const ps_mbf16x8 p_frag = __builtin_convertvector(pf, ps_mbf16x8);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int dt = 0; dt < 2; dt++) {
            const int d = dt * 32 + rc;
            const int vo = ((kt * 2 + j) * 2 + hi) ^ (d & 7);
            ps_mbf16x8 v_frag = ps_as_mbf16_64(
                *(const ps_bf16x8*)(&v_t[buf][d][vo * 8]));
            o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                v_frag, p_frag, o_acc[dt], 0, 0, 0);
          }
          __builtin_amdgcn_s_setprio(0);
        }
      }
    }
    __syncthreads();
  }

  const bool row_ok = wq0 + rc < n_rows;
  const long t = q_tok0 + wq0 + rc;  // dereferenced under row_ok only
  if (n_splits > 1) {
    // ---- epilogue: unnormalised partials for the combiner ----
    if (!row_ok) return;
    if (hi == 0) {
      ws_ml[((long)split * q_tokens + t) * QH + qh] = m_run;
      ws_ml[((long)(n_splits + split) * q_tokens + t) * QH + qh] = l_run;
    }
    float* orow = ws_o + (((long)split * q_tokens + t) * QH + qh) * D;
#pragma unroll
    for (int dt = 0; dt < 2; dt++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        ps_f32x4 o4;
#pragma unroll
        for (int i = 0; i < 4; i++) o4[i] = o_acc[dt][4 * g + i];
        *(ps_f32x4*)(orow + dt * 32 + 8 * g + 4 * hi) = o4;
      }
    return;
  }

  // ---- epilogue: normalise + store. Register quad g of d-tile dt is
  // d = dt*32 + 8g + 4hi + 0..3; the half-waves trade one quad of every
  // pair so that each lane owns 8 consecutive d (16 bytes) ----
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  unsigned short* orow = out + (t * QH + qh) * D;
#pragma unroll
  for (int dt = 0; dt < 2; dt++)
#pragma unroll
    for (int p = 0; p < 2; p++) {
      unsigned int qa[2], qb[2];  // quads g = 2p and g = 2p + 1
#pragma unroll
      for (int i = 0; i < 2; i++) {
        qa[i] = (unsigned int)ps_f32_to_bf16(o_acc[dt][8 * p + 2 * i] * inv) |
                ((unsigned int)ps_f32_to_bf16(
                     o_acc[dt][8 * p + 2 * i + 1] * inv) << 16);
        qb[i] = (unsigned int)ps_f32_to_bf16(
                    o_acc[dt][8 * p + 4 + 2 * i] * inv) |
                ((unsigned int)ps_f32_to_bf16(
                     o_acc[dt][8 * p + 4 + 2 * i + 1] * inv) << 16);
      }
      const unsigned int r0 = __shfl_xor(hi ? qa[0] : qb[0], 32);
      const unsigned int r1 = __shfl_xor(hi ? qa[1] : qb[1], 32);
      ps_u32x4 st;
      if (hi) {  // d = 16p + 8 .. 16p + 15
        st[0] = r0; st[1] = r1; st[2] = qb[0]; st[3] = qb[1];
      } else {   // d = 16p .. 16p + 7
        st[0] = qa[0]; st[1] = qa[1]; st[2] = r0; st[3] = r1;
      }
      if (row_ok) *(ps_u32x4*)(orow + dt * 32 + 16 * p + 8 * hi) = st;
    }
}

// merge the splits: out = sum_s w_s O_s / sum_s w_s l_s, w_s = exp2(m_s - M).
// 16 lanes x 4 dims per (token, head), 16 pairs per workgroup.
__global__ __launch_bounds__(256) void prefill_split_combine64_kernel(
    unsigned short* __restrict__ out,      // [T, QH, 64]
    const float* __restrict__ ws_o,        // [S, T, QH, 64]
    const float* __restrict__ ws_ml,       // [2, S, T, QH]
    long q_tokens, int QH, int n_splits) {
  const long n_th = q_tokens * QH;
  const long th = (long)blockIdx.x * 16 + (threadIdx.x >> 4);  // t * QH + qh
  if (th >= n_th) return;
  const int d4 = (threadIdx.x & 15) * 4;
  float M = PS_NEG_INF;
  for (int s = 0; s < n_splits; s++) M = fmaxf(M, ws_ml[s * n_th + th]);
  float denom = 0.f;
  ps_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < n_splits; s++) {
    const float m = ws_ml[s * n_th + th];
    const float l = ws_ml[(n_splits + s) * n_th + th];
    const float w = (m > PS_NEG_INF && l > 0.f) ? exp2f(m - M) : 0.f;
    denom += w * l;
    const ps_f32x4 o4 = *(const ps_f32x4*)(ws_o + (s * n_th + th) * 64 + d4);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] += w * o4[i];
  }
  ps_bf16x4 r;
#pragma unroll
  for (int i = 0; i < 4; i++)
    r[i] = ps_f32_to_bf16(denom > 0.f ? acc[i] / denom : 0.f);
  *(ps_bf16x4*)(out + th * 64 + d4) = r;
}

extern "C" {

int ps_prefill_mfma32_splits(int num_tiles, int KH, int GQ);

// Same argument list, tiles and split rule as ps_paged_attn_prefill_mfma32.
int ps_paged_attn_prefill_mfma64(void* out, void* ws_o, void* ws_ml,
                                 long q_tokens, const void* q,
                                 const void* k_cache, const void* v_cache,
                                 const void* block_tables,
                                 const void* tile_info, int num_tiles,
                                 int num_q_heads, int max_blocks,
                                 float scale, int KH, int GQ, int head_dim,
                                 long q_stride, int kv_fp8, int window,
                                 hipStream_t stream) {
  if (head_dim != 64) return -1;
  int gqw = 1;
  while (gqw < 4 && GQ % (gqw * 2) == 0) gqw *= 2;
  const int n_work = num_tiles * KH * (GQ / gqw);
  int splits = ps_prefill_mfma32_splits(num_tiles, KH, GQ);
  if (ws_o == nullptr) splits = 1;
  dim3 grid(((n_work + 7) / 8) * 8, splits);
#define PS_PF64_LAUNCH(GQW, KVT)                                          \
  paged_attn_prefill_mfma64_kernel<GQW, KVT>                              \
      <<<grid, 512, 0, stream>>>(                                         \
          (unsigned short*)out, (float*)ws_o, (float*)ws_ml, q_tokens,    \
          (const unsigned short*)q,                                       \
          (const KVT*)k_cache, (const KVT*)v_cache,                       \
          (const int*)block_tables, (const int*)tile_info, max_blocks,    \
          scale, KH, GQ, q_stride, num_q_heads, n_work, window)
  if (kv_fp8) {
    if (gqw == 4) PS_PF64_LAUNCH(4, unsigned char);
    else if (gqw == 2) PS_PF64_LAUNCH(2, unsigned char);
    else PS_PF64_LAUNCH(1, unsigned char);
  } else {
    if (gqw == 4) PS_PF64_LAUNCH(4, unsigned short);
    else if (gqw == 2) PS_PF64_LAUNCH(2, unsigned short);
    else PS_PF64_LAUNCH(1, unsigned short);
  }
#undef PS_PF64_LAUNCH
  if (splits > 1) {
    const long n_th = q_tokens * num_q_heads;
    prefill_split_combine64_kernel<<<
        dim3((unsigned)((n_th + 15) / 16)), 256, 0, stream>>>(
        (unsigned short*)out, (const float*)ws_o, (const float*)ws_ml,
        q_tokens, num_q_heads, splits);
  }
  return 0;
}

}  // extern "C"
