// PyTorch bindings for the MI355X serving kernels (production_stack_amd._C).
//
// The kernels themselves live in *.hip translation units behind a plain C
// ABI (raw pointers + hipStream_t); this file only validates tensors and
// forwards to them on the current HIP stream.
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <vector>

#include "step_pack.h"

extern "C" {
// the row-in-registers launchers return non-zero, launching nothing, when D
// is not a multiple of 8 or exceeds their largest instantiation
int ps_rms_norm(void* out, const void* x, const void* w, float eps, long T,
                int D, hipStream_t stream);
int ps_fused_add_rms_norm(void* x, void* residual, const void* w, float eps,
                          long T, int D, hipStream_t stream);
int ps_rms_norm_fp8(void* out_q, void* out_scale, void* x, void* residual,
                    const void* w, float eps, long T, int D, int fused,
                    hipStream_t stream);
int ps_silu_and_mul_fp8(void* out_q, void* out_scale, const void* x, long T,
                        int D, hipStream_t stream);
void ps_silu_and_mul(void* out, const void* x, long T, int D,
                     hipStream_t stream);
void ps_rope(const void* positions, void* q, void* k, const void* cos_sin,
             long T, int QH, int KH, int HD, int ROT, hipStream_t stream);
void ps_fused_rope_cache(void* qkv, const void* positions, const void* cos_sin,
                         const void* slot_mapping, void* k_cache,
                         void* v_cache, long T, int QH, int KH, int HD,
                         int ROT, long qkv_stride, int BS, int kv_fp8,
                         hipStream_t stream);
int ps_paged_attn_decode(void* out, void* ws_acc, void* ws_ml, const void* q,
                         const void* k_cache, const void* v_cache,
                         const void* block_tables, const void* seq_lens,
                         int num_seqs, int max_blocks, float scale, int KH,
                         int GQ, int head_dim, int block_size, int num_splits,
                         long q_stride, int variant, int kv_fp8, int window,
                         const void* order, hipStream_t stream);
int ps_decode_order(void* order, const void* seq_lens, int S,
                    hipStream_t stream);
int ps_prefill_mfma32_splits(int num_tiles, int KH, int GQ);
int ps_paged_attn_prefill_mfma32(void* out, void* ws_o, void* ws_ml,
                                 long q_tokens, const void* q,
                                 const void* k_cache, const void* v_cache,
                                 const void* block_tables,
                                 const void* tile_info, int num_tiles,
                                 int num_q_heads, int max_blocks,
                                 float scale, int KH, int GQ, int head_dim,
                                 long q_stride, int kv_fp8, int window,
                                 hipStream_t stream);
int ps_paged_attn_prefill_mfma(void* out, const void* q, const void* k_cache,
                               const void* v_cache, const void* block_tables,
                               const void* tile_info, int num_tiles,
                               int num_q_heads, int max_blocks, float scale,
                               int KH, int GQ, int head_dim, long q_stride,
                               int variant, int kv_fp8, int window, hipStream_t stream);
int ps_paged_attn_prefill(void* out, const void* q, const void* k_cache,
                          const void* v_cache, const void* block_tables,
                          const void* token_seq, const void* token_pos,
                          int num_tokens, int num_q_heads, int max_blocks,
                          float scale, int KH, int GQ, int head_dim,
                          int block_size, long q_stride, int window,
                          hipStream_t stream);
void ps_reshape_and_cache(const void* k, const void* v, void* k_cache,
                          void* v_cache, const void* slot_mapping, long T,
                          int KH, int HD, int BS, int kv_fp8,
                          hipStream_t stream);
void ps_greedy_sample(void* out, const void* logits, long R, int V,
                      hipStream_t stream);
void ps_kv_quant(void* out, void* scales, const void* in, long rows, int hd,
                 hipStream_t stream);
void ps_kv_dequant(void* out, const void* in, const void* scales, long rows,
                   int hd, hipStream_t stream);
int ps_skinny_gemm_splits(int M, int N, int K);
int ps_skinny_gemm(void* out_bf16, void* ws, const void* x, const void* w,
                   int M, int N, int K, long x_stride, hipStream_t stream);
int ps_skinny_gemm_fp8_splits(int M, int N, int K);
int ps_skinny_gemm_fp8(void* out_bf16, void* ws, const void* xq,
                       const void* sx, const void* wq, const void* sw, int M,
                       int N, int K, hipStream_t stream);
int ps_skinny_gemm_w4_splits(int M, int N, int K);
int ps_skinny_gemm_w4(void* out_bf16, void* ws, const void* x,
                      const void* packed, const void* scales,
                      const void* zeros, int M, int N, int K,
                      hipStream_t stream);
int ps_int4_dequant(void* out_bf16, const void* packed, const void* scales,
                    const void* zeros, long N, int K, hipStream_t stream);
int ps_quant_fp8_rows(void* out_q, void* out_scale, const void* x, long T,
                      int D, long x_stride, hipStream_t stream);
int ps_gemm8p_splits(int M, int N, int K);
int ps_gemm8p(void* out_bf16, void* ws, const void* x, const void* w, int M,
              int N, int K, long x_stride, hipStream_t stream);
int ps_lora_bgmv(void* out, const void* x, const void* A, const void* B,
                 const void* scale, const void* idx, int T, int IN, int W,
                 int R, long out_stride, long x_stride, int col_off,
                 hipStream_t stream);
int ps_fused_moe_supported(int T, int top_k, int E, int H, int I);
int ps_fused_moe(void* out, void* offsets, void* sorted_pairs, void* act,
                 void* y, const void* x, const void* w_gate_up,
                 const void* w_down, const void* topk_ids, int ids_i64,
                 const void* topk_w, int T, int top_k, int E, int H, int I,
                 hipStream_t stream);
int ps_resolve_placeholders(void* tokens, const void* prev_row,
                            const void* prev_tokens, long n, long n_prev,
                            hipStream_t stream);
}

at::Tensor cachegen_encode(at::Tensor q);
at::Tensor cachegen_decode(at::Tensor blob, int64_t hd);

namespace {

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_GPU_BF16(t)                                             \
  TORCH_CHECK((t).is_cuda(), #t " must be on the GPU");               \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16"); \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

#define CHECK_GPU_DTYPE(t, ty)                                  \
  TORCH_CHECK((t).is_cuda(), #t " must be on the GPU");         \
  TORCH_CHECK((t).scalar_type() == (ty), #t " dtype mismatch"); \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// [T] fp32 row scales and [T, D] fp8 codes written by the act-quant kernels
void check_fp8_outputs(const at::Tensor& out_q, const at::Tensor& scales,
                       long T, long D) {
  TORCH_CHECK(out_q.is_cuda() && out_q.is_contiguous(),
              "out_q must be GPU-contiguous");
  TORCH_CHECK(out_q.scalar_type() == at::kFloat8_e4m3fn ||
                  out_q.scalar_type() == at::kByte,
              "out_q must be fp8/byte");
  TORCH_CHECK(out_q.dim() == 2 && out_q.size(0) == T && out_q.size(1) == D,
              "out_q must be [", T, ", ", D, "]");
  CHECK_GPU_DTYPE(scales, at::kFloat);
  TORCH_CHECK(scales.numel() == T, "scales must hold one value per row");
}

// rotary width taken from the cos/sin table: pairs (r, r + ROT/2) inside the
// leading ROT dims of each head
int rotary_dim(const at::Tensor& cos_sin, int HD) {
  TORCH_CHECK(cos_sin.dim() == 2, "cos_sin must be [max_pos, rot_dim]");
  const long ROT = cos_sin.size(1);
  TORCH_CHECK(ROT >= 0 && ROT % 2 == 0, "rot_dim must be even, got ", ROT);
  TORCH_CHECK(ROT <= HD, "rot_dim ", ROT, " exceeds head_dim ", HD);
  return (int)ROT;
}

// KV caches are bf16 or OCP fp8 e4m3; returns 1 for fp8
int cache_fp8(const at::Tensor& c) {
  TORCH_CHECK(c.is_cuda() && c.is_contiguous(), "cache must be GPU-contig");
  if (c.scalar_type() == at::kBFloat16) return 0;
  if (c.scalar_type() == at::kFloat8_e4m3fn) return 1;
  TORCH_CHECK(false, "KV cache must be bf16 or float8_e4m3fn");
  return 0;
}

// q may be a row-strided view into the packed qkv tensor
long q_row_stride(const at::Tensor& q, int HD) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "q must be bf16 on GPU");
  TORCH_CHECK(q.dim() == 3 && q.stride(2) == 1 && q.stride(1) == HD,
              "q must be [T, H, HD] with contiguous heads");
  return q.stride(0);
}

void rms_norm(at::Tensor out, at::Tensor x, at::Tensor w, double eps) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_BF16(x);
  CHECK_GPU_BF16(w);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, "x must be [..., D], D > 0");
  const long T = x.numel() / x.size(-1);
  const int D = (int)x.size(-1);
  TORCH_CHECK(D % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(out.sizes() == x.sizes(), "out must have x's shape");
  TORCH_CHECK(w.numel() == D, "w must hold D=", D, " weights");
  int rc = ps_rms_norm(out.data_ptr(), x.data_ptr(), w.data_ptr(), (float)eps,
                       T, D, current_stream());
  TORCH_CHECK(rc == 0, "rms_norm: unsupported hidden dim ", D);
}

void fused_add_rms_norm(at::Tensor x, at::Tensor residual, at::Tensor w,
                        double eps) {
  CHECK_GPU_BF16(x);
  CHECK_GPU_BF16(residual);
  CHECK_GPU_BF16(w);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, "x must be [..., D], D > 0");
  const long T = x.numel() / x.size(-1);
  const int D = (int)x.size(-1);
  TORCH_CHECK(D % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(residual.sizes() == x.sizes(), "residual must have x's shape");
  TORCH_CHECK(w.numel() == D, "w must hold D=", D, " weights");
  int rc = ps_fused_add_rms_norm(x.data_ptr(), residual.data_ptr(),
                                 w.data_ptr(), (float)eps, T, D,
                                 current_stream());
  TORCH_CHECK(rc == 0, "fused_add_rms_norm: unsupported hidden dim ", D);
}

void silu_and_mul(at::Tensor out, at::Tensor x) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_BF16(x);
  TORCH_CHECK(out.dim() >= 1 && out.size(-1) > 0, "out must be [..., D]");
  const int D = (int)out.size(-1);
  TORCH_CHECK(x.size(-1) == 2 * D, "x last dim must be 2*out last dim");
  TORCH_CHECK(D % 8 == 0, "feature dim must be a multiple of 8");
  const long T = out.numel() / D;
  TORCH_CHECK(x.numel() == 2 * T * D, "x must be [..., 2*D] over out's rows");
  ps_silu_and_mul(out.data_ptr(), x.data_ptr(), T, D, current_stream());
}

void rotary_embedding(at::Tensor positions, at::Tensor q, at::Tensor k,
                      at::Tensor cos_sin, long head_dim) {
  CHECK_GPU_DTYPE(positions, at::kInt);
  CHECK_GPU_BF16(q);
  CHECK_GPU_BF16(k);
  CHECK_GPU_DTYPE(cos_sin, at::kFloat);
  const long T = positions.numel();
  TORCH_CHECK(head_dim > 0, "head_dim must be positive");
  const int HD = (int)head_dim;
  const int ROT = rotary_dim(cos_sin, HD);
  if (T == 0) return;
  TORCH_CHECK(q.numel() % (T * HD) == 0 && k.numel() % (T * HD) == 0,
              "q/k must be [T, H*head_dim]");
  const int QH = (int)(q.numel() / T / HD);
  const int KH = (int)(k.numel() / T / HD);
  ps_rope(positions.data_ptr(), q.data_ptr(), k.data_ptr(),
          cos_sin.data_ptr(), T, QH, KH, HD, ROT, current_stream());
}

void paged_attn_decode(at::Tensor out, at::Tensor q, at::Tensor k_cache,
                       at::Tensor v_cache, at::Tensor block_tables,
                       at::Tensor seq_lens, double scale, int64_t num_splits,
                       int64_t variant, int64_t window,
                       c10::optional<at::Tensor> order) {
  CHECK_GPU_BF16(out);
  const int kv_fp8 = cache_fp8(k_cache);
  cache_fp8(v_cache);
  CHECK_GPU_DTYPE(block_tables, at::kInt);
  CHECK_GPU_DTYPE(seq_lens, at::kInt);
  const int S = (int)q.size(0);
  // launch order of the sequences (ops.decode_order): a permutation of
  // [0, S). The kernel skips entries outside [0, S).
  const void* order_p = nullptr;
  if (order.has_value()) {
    const at::Tensor& order_t = *order;
    CHECK_GPU_DTYPE(order_t, at::kInt);
    TORCH_CHECK(order_t.numel() == S, "order must have one entry per seq");
    order_p = order_t.data_ptr();
  }
  const int QH = (int)q.size(1);
  const int HD = (int)q.size(2);
  const int KH = (int)k_cache.size(1);
  const int BS = (int)k_cache.size(2);
  TORCH_CHECK(QH % KH == 0, "GQA group mismatch");
  const int GQ = QH / KH;
  const int max_blocks = (int)block_tables.size(1);
  if (num_splits <= 0) {
    // fill ~3 workgroups per CU, bounded by useful split granularity
    const int target = 2048;
    num_splits = std::min<int64_t>(
        32, std::max<int64_t>(1, target / std::max(1, S * KH)));
  }
  at::Tensor ws_acc, ws_ml;
  void *acc_p = nullptr, *ml_p = nullptr;
  if (num_splits > 1) {
    auto opts = q.options().dtype(at::kFloat);
    ws_acc = at::empty({(long)S * QH * num_splits * HD}, opts);
    ws_ml = at::empty({(long)S * QH * num_splits * 2}, opts);
    acc_p = ws_acc.data_ptr();
    ml_p = ws_ml.data_ptr();
  }
  int rc = ps_paged_attn_decode(
      out.data_ptr(), acc_p, ml_p, q.data_ptr(), k_cache.data_ptr(),
      v_cache.data_ptr(), block_tables.data_ptr(), seq_lens.data_ptr(), S,
      max_blocks, (float)scale, KH, GQ, HD, BS, (int)num_splits,
      q_row_stride(q, HD), (int)variant, kv_fp8, (int)window, order_p,
      current_stream());
  TORCH_CHECK(rc == 0, "unsupported decode config: head_dim=", HD,
              " block_size=", BS, " gqa=", GQ, " variant=", variant);
}

// order <- stable descending argsort of seq_lens; false (order untouched)
// when S is outside what the kernel handles
bool decode_order(at::Tensor order, at::Tensor seq_lens) {
  CHECK_GPU_DTYPE(order, at::kInt);
  CHECK_GPU_DTYPE(seq_lens, at::kInt);
  TORCH_CHECK(order.numel() == seq_lens.numel(), "order/seq_lens size");
  return ps_decode_order(order.data_ptr(), seq_lens.data_ptr(),
                         (int)seq_lens.numel(), current_stream()) == 0;
}

// Host checks shared by the two prefill bindings (no device read): q is
// [T, QH, hd] bf16 with contiguous heads (rows may be strided), out is
// [T, QH, hd], K and V agree and carry hd, window is not negative.
void check_prefill_args(const at::Tensor& out, const at::Tensor& q,
                        const at::Tensor& k_cache, const at::Tensor& v_cache,
                        const at::Tensor& block_tables, int64_t window) {
  TORCH_CHECK(q.dim() == 3, "q must be [T, QH, head_dim]");
  q_row_stride(q, (int)q.size(2));
  TORCH_CHECK(out.sizes() == q.sizes(), "out must be [T, QH, head_dim]");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes() &&
                  k_cache.scalar_type() == v_cache.scalar_type(),
              "k_cache and v_cache must be [NB, KH, BS, head_dim] of one "
              "shape and dtype");
  TORCH_CHECK(k_cache.size(3) == q.size(2),
              "cache head_dim ", k_cache.size(3), " != q head_dim ",
              q.size(2));
  TORCH_CHECK(block_tables.dim() == 2,
              "block_tables must be [num_seqs, max_blocks]");
  TORCH_CHECK(window >= 0, "window must be >= 0, got ", window);
}

void paged_attn_prefill(at::Tensor out, at::Tensor q, at::Tensor k_cache,
                        at::Tensor v_cache, at::Tensor block_tables,
                        at::Tensor token_seq, at::Tensor token_pos,
                        double scale, int64_t window) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_BF16(k_cache);
  CHECK_GPU_BF16(v_cache);
  CHECK_GPU_DTYPE(block_tables, at::kInt);
  CHECK_GPU_DTYPE(token_seq, at::kInt);
  CHECK_GPU_DTYPE(token_pos, at::kInt);
  check_prefill_args(out, q, k_cache, v_cache, block_tables, window);
  const int T = (int)q.size(0);
  const int QH = (int)q.size(1);
  const int HD = (int)q.size(2);
  const int KH = (int)k_cache.size(1);
  const int BS = (int)k_cache.size(2);
  TORCH_CHECK(token_seq.numel() == T && token_pos.numel() == T,
              "token_seq/token_pos must hold one entry per q row");
  TORCH_CHECK(QH % KH == 0, "GQA group mismatch");
  const int GQ = QH / KH;
  const int max_blocks = (int)block_tables.size(1);
  if (T == 0) return;
  int rc = ps_paged_attn_prefill(
      out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      block_tables.data_ptr(), token_seq.data_ptr(), token_pos.data_ptr(), T,
      QH, max_blocks, (float)scale, KH, GQ, HD, BS, q_row_stride(q, HD),
      (int)window, current_stream());
  TORCH_CHECK(rc == 0, "unsupported prefill config: head_dim=", HD,
              " block_size=", BS);
}

void paged_attn_prefill_mfma(at::Tensor out, at::Tensor q,
                             at::Tensor k_cache, at::Tensor v_cache,
                             at::Tensor block_tables, at::Tensor tile_info,
                             double scale, int64_t variant, int64_t window) {
  CHECK_GPU_BF16(out);
  const int kv_fp8 = cache_fp8(k_cache);
  cache_fp8(v_cache);
  CHECK_GPU_DTYPE(block_tables, at::kInt);
  CHECK_GPU_DTYPE(tile_info, at::kInt);
  check_prefill_args(out, q, k_cache, v_cache, block_tables, window);
  TORCH_CHECK(tile_info.dim() == 2 && tile_info.size(1) == 4,
              "tile_info must be [num_tiles, 4]");
  TORCH_CHECK(variant >= 3 && variant <= 5,
              "mfma prefill variant must be 3, 4 or 5, got ", variant);
  const int QH = (int)q.size(1);
  const int HD = (int)q.size(2);
  const int KH = (int)k_cache.size(1);
  TORCH_CHECK(QH % KH == 0, "GQA group mismatch");
  TORCH_CHECK(k_cache.size(2) == 16, "mfma prefill needs block_size 16");
  const int GQ = QH / KH;
  const int NT = (int)tile_info.size(0);
  if (NT == 0) return;
  int rc;
  if (variant == 5) {
    // v5 with split-KV: allocate fp32 partial workspace when the launch
    // is small enough that the splits heuristic fires
    const int splits = ps_prefill_mfma32_splits(NT, KH, QH / KH);
    const long T = q.size(0);
    void *ws_o_p = nullptr, *ws_ml_p = nullptr;
    at::Tensor ws_o, ws_ml;
    if (splits > 1) {
      ws_o = at::empty({(long)splits * T * QH * HD},
                       q.options().dtype(at::kFloat));
      ws_ml = at::empty({2L * splits * T * QH},
                        q.options().dtype(at::kFloat));
      ws_o_p = ws_o.data_ptr();
      ws_ml_p = ws_ml.data_ptr();
    }
    rc = ps_paged_attn_prefill_mfma32(
        out.data_ptr(), ws_o_p, ws_ml_p, T, q.data_ptr(),
        k_cache.data_ptr(), v_cache.data_ptr(), block_tables.data_ptr(),
        tile_info.data_ptr(), NT, QH, (int)block_tables.size(1),
        (float)scale, KH, QH / KH, HD, q_row_stride(q, HD), kv_fp8,
        (int)window, current_stream());
  } else {
    rc = ps_paged_attn_prefill_mfma(
        out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
        v_cache.data_ptr(), block_tables.data_ptr(), tile_info.data_ptr(),
        NT, QH, (int)block_tables.size(1), (float)scale, KH, GQ, HD,
        q_row_stride(q, HD), (int)variant, kv_fp8, (int)window,
        current_stream());
  }
  TORCH_CHECK(rc == 0, "unsupported mfma prefill config: head_dim=", HD);
}

void fused_rope_cache(at::Tensor qkv, at::Tensor positions,
                      at::Tensor cos_sin, at::Tensor slot_mapping,
                      at::Tensor k_cache, at::Tensor v_cache,
                      int64_t q_heads, int64_t head_dim) {
  CHECK_GPU_BF16(qkv);
  CHECK_GPU_DTYPE(positions, at::kInt);
  CHECK_GPU_DTYPE(cos_sin, at::kFloat);
  CHECK_GPU_DTYPE(slot_mapping, at::kLong);
  const int kv_fp8 = cache_fp8(k_cache);
  cache_fp8(v_cache);
  const long T = positions.numel();
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
                  v_cache.scalar_type() == k_cache.scalar_type(),
              "k/v cache must both be [NB, KH, BS, HD] of one dtype");
  const int KH = (int)k_cache.size(1);
  const int BS = (int)k_cache.size(2);
  TORCH_CHECK(head_dim > 0 && head_dim % 8 == 0,
              "head_dim must be a positive multiple of 8");
  const int HD = (int)head_dim;
  TORCH_CHECK(k_cache.size(3) == HD, "cache head_dim mismatch");
  const int ROT = rotary_dim(cos_sin, HD);
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == T &&
                  qkv.size(1) == (q_heads + 2 * KH) * HD,
              "qkv must be [T, (q_heads + 2*KH) * head_dim]");
  TORCH_CHECK(slot_mapping.numel() == T, "one slot per token");
  if (T == 0) return;
  ps_fused_rope_cache(qkv.data_ptr(), positions.data_ptr(),
                      cos_sin.data_ptr(), slot_mapping.data_ptr(),
                      k_cache.data_ptr(), v_cache.data_ptr(), T,
                      (int)q_heads, KH, HD, ROT, qkv.stride(0), BS, kv_fp8,
                      current_stream());
}

void reshape_and_cache(at::Tensor k, at::Tensor v, at::Tensor k_cache,
                       at::Tensor v_cache, at::Tensor slot_mapping) {
  CHECK_GPU_BF16(k);
  CHECK_GPU_BF16(v);
  const int kv_fp8 = cache_fp8(k_cache);
  cache_fp8(v_cache);
  CHECK_GPU_DTYPE(slot_mapping, at::kLong);
  const long T = slot_mapping.numel();
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
                  v_cache.scalar_type() == k_cache.scalar_type(),
              "k/v cache must both be [NB, KH, BS, HD] of one dtype");
  const int KH = (int)k_cache.size(1);
  const int BS = (int)k_cache.size(2);
  const int HD = (int)k_cache.size(3);
  TORCH_CHECK(HD % 8 == 0, "head_dim must be a multiple of 8");
  TORCH_CHECK(k.numel() == T * KH * HD, "k shape mismatch");
  TORCH_CHECK(v.numel() == T * KH * HD, "v shape mismatch");
  if (T == 0) return;
  ps_reshape_and_cache(k.data_ptr(), v.data_ptr(), k_cache.data_ptr(),
                       v_cache.data_ptr(), slot_mapping.data_ptr(), T, KH, HD,
                       BS, kv_fp8, current_stream());
}

// The fp32 split-K workspace ws[splits, M, N] of a GEMM, on `like`'s device:
// allocated into `ws` and returned as a pointer, null when splits <= 1.
void* splitk_workspace(at::Tensor& ws, const at::Tensor& like, int splits,
                       int M, int N) {
  if (splits <= 1) return nullptr;
  ws = at::empty({(long)splits * M * N}, like.options().dtype(at::kFloat));
  return ws.data_ptr();
}

// out[M, N] = x[M, K] @ w[N, K]^T in bf16 on one device; x may be a
// row-strided view. skinny_gemm and gemm8p both read x and w as 16-byte
// vectors at multiples of 8 elements from a row start. Sets M, N, K.
void check_bf16_gemm(const at::Tensor& out, const at::Tensor& x,
                     const at::Tensor& w, int& M, int& N, int& K) {
  CHECK_GPU_BF16(out);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "x must be bf16");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be 2D row-major");
  CHECK_GPU_BF16(w);
  TORCH_CHECK(w.dim() == 2, "w must be [N, K]");
  M = (int)x.size(0);
  K = (int)x.size(1);
  N = (int)w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N,
              "out must be [", M, ", ", N, "]");
  TORCH_CHECK(x.device() == w.device() && out.device() == x.device(),
              "out, x and w must be on one device");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)w.data_ptr() % 16 == 0,
              "x and w rows must be 16-byte aligned");
  TORCH_CHECK(M <= 1 || x.stride(0) % 8 == 0,
              "x row stride must be a multiple of 8 elements");
}

void skinny_gemm(at::Tensor out, at::Tensor x, at::Tensor w) {
  int M, N, K;
  check_bf16_gemm(out, x, w, M, N, K);
  const int splits = ps_skinny_gemm_splits(M, N, K);
  TORCH_CHECK(splits > 0, "unsupported skinny gemm shape M=", M, " N=", N,
              " K=", K);
  at::Tensor ws;
  void* ws_p = splitk_workspace(ws, x, splits, M, N);
  int rc = ps_skinny_gemm(out.data_ptr(), ws_p, x.data_ptr(), w.data_ptr(),
                          M, N, K, x.stride(0), current_stream());
  TORCH_CHECK(rc == 0, "skinny gemm launch failed");
}

void rms_norm_fp8(at::Tensor out_q, at::Tensor scales, at::Tensor x,
                  at::Tensor residual, at::Tensor w, double eps,
                  int64_t fused) {
  CHECK_GPU_BF16(x);
  CHECK_GPU_BF16(w);
  TORCH_CHECK(x.dim() == 2, "x must be [T, D]");
  const long T = x.size(0);
  const int D = (int)x.size(1);
  TORCH_CHECK(D % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(w.numel() == D, "w must hold D=", D, " weights");
  check_fp8_outputs(out_q, scales, T, D);
  if (fused) {
    CHECK_GPU_BF16(residual);
    TORCH_CHECK(residual.sizes() == x.sizes(), "residual must have x's shape");
  }
  int rc = ps_rms_norm_fp8(out_q.data_ptr(), scales.data_ptr(), x.data_ptr(),
                           fused ? residual.data_ptr() : nullptr,
                           w.data_ptr(), (float)eps, T, D, (int)fused,
                           current_stream());
  TORCH_CHECK(rc == 0, "rms_norm_fp8: unsupported hidden dim ", D);
}

void silu_and_mul_fp8(at::Tensor out_q, at::Tensor scales, at::Tensor x) {
  CHECK_GPU_BF16(x);
  TORCH_CHECK(x.dim() == 2 && x.size(1) % 2 == 0, "x must be [T, 2*D]");
  const long T = x.size(0);
  const int D = (int)(x.size(1) / 2);
  TORCH_CHECK(D % 8 == 0, "feature dim must be a multiple of 8");
  check_fp8_outputs(out_q, scales, T, D);
  int rc = ps_silu_and_mul_fp8(out_q.data_ptr(), scales.data_ptr(),
                               x.data_ptr(), T, D, current_stream());
  TORCH_CHECK(rc == 0, "silu_and_mul_fp8: unsupported feature dim ", D);
}

void quant_fp8_rows(at::Tensor out_q, at::Tensor scales, at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "x must be bf16 on the GPU");
  TORCH_CHECK(x.dim() == 2 && (x.size(1) <= 1 || x.stride(1) == 1),
              "x must be [T, D] with contiguous rows");
  const long T = x.size(0);
  const int D = (int)x.size(1);
  TORCH_CHECK(D > 0 && D % 8 == 0, "feature dim must be a multiple of 8");
  // rows are read as 16-byte vectors
  TORCH_CHECK(T <= 1 || x.stride(0) % 8 == 0,
              "x row stride must be a multiple of 8 elements");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0,
              "x rows must be 16-byte aligned");
  check_fp8_outputs(out_q, scales, T, D);
  int rc = ps_quant_fp8_rows(out_q.data_ptr(), scales.data_ptr(),
                             x.data_ptr(), T, D, T > 1 ? x.stride(0) : D,
                             current_stream());
  TORCH_CHECK(rc == 0, "quant_fp8_rows: unsupported feature dim ", D);
}

void skinny_gemm_fp8(at::Tensor out, at::Tensor xq, at::Tensor sx,
                     at::Tensor wq, at::Tensor sw) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_DTYPE(xq, at::kFloat8_e4m3fn);
  CHECK_GPU_DTYPE(wq, at::kFloat8_e4m3fn);
  CHECK_GPU_DTYPE(sx, at::kFloat);
  CHECK_GPU_DTYPE(sw, at::kFloat);
  TORCH_CHECK(xq.dim() == 2 && wq.dim() == 2, "xq and wq must be 2D");
  const int M = (int)xq.size(0);
  const int K = (int)xq.size(1);
  const int N = (int)wq.size(0);
  TORCH_CHECK(xq.size(0) <= 256, "unsupported skinny fp8 gemm M=",
              xq.size(0));
  TORCH_CHECK(wq.size(1) == K, "K mismatch");
  TORCH_CHECK(sx.numel() == M, "sx must hold one scale per row of xq");
  TORCH_CHECK(sw.numel() == N, "sw must hold one scale per row of wq");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N,
              "out must be [", M, ", ", N, "]");
  const int splits = ps_skinny_gemm_fp8_splits(M, N, K);
  TORCH_CHECK(splits > 0, "unsupported skinny fp8 gemm shape M=", M, " N=", N,
              " K=", K);
  // rows are read as 16-byte vectors; K % 64 == 0 keeps every row start
  // aligned once the base is
  TORCH_CHECK((uintptr_t)xq.data_ptr() % 16 == 0 &&
                  (uintptr_t)wq.data_ptr() % 16 == 0,
              "xq and wq rows must be 16-byte aligned");
  at::Tensor ws;
  void* ws_p = splitk_workspace(ws, xq, splits, M, N);
  int rc = ps_skinny_gemm_fp8(out.data_ptr(), ws_p, xq.data_ptr(),
                              sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), M,
                              N, K, current_stream());
  TORCH_CHECK(rc == 0, "skinny fp8 gemm launch failed");
}

// packed [N, K/2] uint8, s [N, K/128] bf16, z [N, K/128] uint8 of one int4
// weight; returns (N, K)
std::pair<long, long> check_int4_weight(const at::Tensor& packed,
                                        const at::Tensor& s,
                                        const at::Tensor& z) {
  CHECK_GPU_DTYPE(packed, at::kByte);
  CHECK_GPU_BF16(s);
  CHECK_GPU_DTYPE(z, at::kByte);
  TORCH_CHECK(packed.dim() == 2, "packed must be [N, K/2]");
  const long N = packed.size(0);
  const long K = packed.size(1) * 2;
  TORCH_CHECK(K >= 128 && K % 128 == 0,
              "K must be a multiple of the int4 group size 128, got ", K);
  TORCH_CHECK(s.dim() == 2 && s.size(0) == N && s.size(1) == K / 128,
              "s must be [", N, ", ", K / 128, "]");
  TORCH_CHECK(z.dim() == 2 && z.size(0) == N && z.size(1) == K / 128,
              "z must be [", N, ", ", K / 128, "]");
  TORCH_CHECK(packed.device() == s.device() && packed.device() == z.device(),
              "packed, s and z must be on one device");
  // rows are read as 16-byte vectors; K % 128 == 0 keeps every row start
  // aligned once the base is
  TORCH_CHECK((uintptr_t)packed.data_ptr() % 16 == 0,
              "packed rows must be 16-byte aligned");
  return {N, K};
}

void skinny_gemm_w4(at::Tensor out, at::Tensor x, at::Tensor packed,
                    at::Tensor s, at::Tensor z) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_BF16(x);
  TORCH_CHECK(x.dim() == 2, "x must be [M, K]");
  const auto nk = check_int4_weight(packed, s, z);
  const int M = (int)x.size(0);
  const int N = (int)nk.first;
  const int K = (int)nk.second;
  TORCH_CHECK(x.size(0) <= 256, "unsupported skinny w4 gemm M=", x.size(0));
  TORCH_CHECK(x.size(1) == K, "K mismatch");
  TORCH_CHECK(x.device() == packed.device() && out.device() == x.device(),
              "out, x and the weight must be on one device");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N,
              "out must be [", M, ", ", N, "]");
  const int splits = ps_skinny_gemm_w4_splits(M, N, K);
  TORCH_CHECK(splits > 0, "unsupported skinny w4 gemm shape M=", M, " N=", N,
              " K=", K);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0,
              "x rows must be 16-byte aligned");
  at::Tensor ws;
  void* ws_p = splitk_workspace(ws, x, splits, M, N);
  int rc = ps_skinny_gemm_w4(out.data_ptr(), ws_p, x.data_ptr(),
                             packed.data_ptr(), s.data_ptr(), z.data_ptr(),
                             M, N, K, current_stream());
  TORCH_CHECK(rc == 0, "skinny w4 gemm launch failed");
}

void int4_dequant(at::Tensor out, at::Tensor packed, at::Tensor s,
                  at::Tensor z) {
  CHECK_GPU_BF16(out);
  const auto nk = check_int4_weight(packed, s, z);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == nk.first &&
                  out.size(1) == nk.second,
              "out must be [", nk.first, ", ", nk.second, "]");
  TORCH_CHECK(out.device() == packed.device(),
              "out and the weight must be on one device");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0,
              "out rows must be 16-byte aligned");
  if (nk.first == 0) return;
  int rc = ps_int4_dequant(out.data_ptr(), packed.data_ptr(), s.data_ptr(),
                           z.data_ptr(), nk.first, (int)nk.second,
                           current_stream());
  TORCH_CHECK(rc == 0, "int4_dequant: unsupported shape");
}

void gemm8p(at::Tensor out, at::Tensor x, at::Tensor w) {
  int M, N, K;
  check_bf16_gemm(out, x, w, M, N, K);
  const int splits = ps_gemm8p_splits(M, N, K);
  TORCH_CHECK(splits > 0, "unsupported gemm8p shape M=", M, " N=", N,
              " K=", K);
  at::Tensor ws;
  void* ws_p = splitk_workspace(ws, x, splits, M, N);
  int rc = ps_gemm8p(out.data_ptr(), ws_p, x.data_ptr(), w.data_ptr(), M, N,
                     K, x.stride(0), current_stream());
  TORCH_CHECK(rc == 0, "gemm8p launch failed");
}

void lora_bgmv(at::Tensor out, at::Tensor x, at::Tensor A, at::Tensor B,
               at::Tensor scale, at::Tensor idx, long col_off) {
  // out and x may be row-strided views of wider buffers
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16,
              "out must be bf16 on the GPU");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "x must be bf16 on the GPU");
  CHECK_GPU_BF16(A);
  CHECK_GPU_BF16(B);
  CHECK_GPU_DTYPE(scale, at::kFloat);
  CHECK_GPU_DTYPE(idx, at::kInt);
  TORCH_CHECK(out.dim() == 2 && out.stride(1) == 1, "out 2D row-major");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x 2D row-major");
  TORCH_CHECK(A.dim() == 3 && A.is_contiguous(), "A [S,R,IN] contiguous");
  TORCH_CHECK(B.dim() == 3 && B.is_contiguous(), "B [S,W,R] contiguous");
  const int T = (int)x.size(0);
  const int IN = (int)x.size(1);
  const int R = (int)A.size(1);
  const int W = (int)B.size(1);
  TORCH_CHECK(A.size(2) == IN, "A IN mismatch");
  TORCH_CHECK(B.size(2) == R, "B R mismatch");
  TORCH_CHECK(out.size(0) == T && idx.numel() == T, "T mismatch");
  TORCH_CHECK(col_off >= 0 && col_off + W <= out.size(1),
              "col range out of bounds");
  TORCH_CHECK(A.size(0) == B.size(0) && scale.numel() == A.size(0),
              "A, B and scale must agree on the slot count");
  TORCH_CHECK(IN % 8 == 0, "IN must be a multiple of 8, got ", IN);
  TORCH_CHECK(x.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "x rows must start on 16-byte boundaries");
  TORCH_CHECK(R >= 1 && R <= 64, "lora_bgmv supports rank 1..64, got ", R);
  if (T == 0) return;
  int rc = ps_lora_bgmv(out.data_ptr(), x.data_ptr(), A.data_ptr(),
                        B.data_ptr(), scale.data_ptr(), idx.data_ptr(), T,
                        IN, W, R, out.stride(0), x.stride(0), (int)col_off,
                        current_stream());
  TORCH_CHECK(rc == 0, "lora_bgmv launch rejected: R=", R, " IN=", IN);
}

bool fused_moe_supported(int64_t T, int64_t top_k, int64_t E, int64_t H,
                         int64_t I) {
  const int64_t lim = 1 << 30;
  if (T > lim || top_k > lim || E > lim || H > lim || I > lim) return false;
  return ps_fused_moe_supported((int)T, (int)top_k, (int)E, (int)H,
                                (int)I) != 0;
}

// scratch tensors come from the caller so they land in the graph pool
// under capture
void fused_moe(at::Tensor out, at::Tensor offsets, at::Tensor sorted_pairs,
               at::Tensor act, at::Tensor y, at::Tensor x,
               at::Tensor experts_gate_up, at::Tensor experts_down,
               at::Tensor topk_ids, at::Tensor topk_w) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_BF16(x);
  CHECK_GPU_BF16(experts_gate_up);
  CHECK_GPU_BF16(experts_down);
  CHECK_GPU_BF16(act);
  CHECK_GPU_DTYPE(y, at::kFloat);
  CHECK_GPU_DTYPE(offsets, at::kInt);
  CHECK_GPU_DTYPE(sorted_pairs, at::kInt);
  CHECK_GPU_DTYPE(topk_w, at::kFloat);
  TORCH_CHECK(topk_ids.is_cuda() && topk_ids.is_contiguous() &&
                  (topk_ids.scalar_type() == at::kLong ||
                   topk_ids.scalar_type() == at::kInt),
              "topk_ids must be contiguous int32/int64 on the GPU");
  TORCH_CHECK(x.dim() == 2 && topk_ids.dim() == 2 &&
                  experts_gate_up.dim() == 3 && experts_down.dim() == 3,
              "fused_moe: x [T,H], topk_ids [T,k], gate_up [E,2I,H], "
              "down [E,H,I]");
  const int64_t T = x.size(0), H = x.size(1);
  const int64_t top_k = topk_ids.size(1);
  const int64_t E = experts_gate_up.size(0);
  const int64_t I = experts_down.size(2);
  TORCH_CHECK(topk_ids.size(0) == T && topk_w.dim() == 2 &&
                  topk_w.size(0) == T && topk_w.size(1) == top_k,
              "fused_moe: routing shape mismatch");
  TORCH_CHECK(experts_gate_up.size(1) == 2 * I &&
                  experts_gate_up.size(2) == H &&
                  experts_down.size(0) == E && experts_down.size(1) == H,
              "fused_moe: expert weight shape mismatch");
  TORCH_CHECK(fused_moe_supported(T, top_k, E, H, I),
              "unsupported fused_moe shape T=", T, " top_k=", top_k, " E=", E,
              " H=", H, " I=", I);
  const int64_t P = T * top_k;
  TORCH_CHECK(out.numel() == T * H && offsets.numel() >= E + 1 &&
                  sorted_pairs.numel() >= P && act.numel() >= P * I &&
                  y.numel() >= P * H,
              "fused_moe: output/scratch too small");
  int rc = ps_fused_moe(
      out.data_ptr(), offsets.data_ptr(), sorted_pairs.data_ptr(),
      act.data_ptr(), y.data_ptr(), x.data_ptr(), experts_gate_up.data_ptr(),
      experts_down.data_ptr(), topk_ids.data_ptr(),
      topk_ids.scalar_type() == at::kLong ? 1 : 0, topk_w.data_ptr(), (int)T,
      (int)top_k, (int)E, (int)H, (int)I, current_stream());
  TORCH_CHECK(rc == 0, "fused_moe launch rejected");
}

void kv_quant(at::Tensor out, at::Tensor scales, at::Tensor in) {
  CHECK_GPU_DTYPE(out, at::kChar);
  CHECK_GPU_DTYPE(scales, at::kFloat);
  CHECK_GPU_BF16(in);
  TORCH_CHECK(in.dim() >= 1 && in.size(-1) > 0, "in must be [..., hd]");
  const int hd = (int)in.size(-1);
  TORCH_CHECK(hd % 8 == 0, "row width must be multiple of 8");
  const long rows = in.numel() / hd;
  TORCH_CHECK(out.sizes() == in.sizes(), "out must have in's shape");
  TORCH_CHECK(scales.numel() == rows, "scales must hold one value per row");
  if (rows == 0) return;
  ps_kv_quant(out.data_ptr(), scales.data_ptr(), in.data_ptr(), rows, hd,
              current_stream());
}

void kv_dequant(at::Tensor out, at::Tensor in, at::Tensor scales) {
  CHECK_GPU_BF16(out);
  CHECK_GPU_DTYPE(in, at::kChar);
  CHECK_GPU_DTYPE(scales, at::kFloat);
  TORCH_CHECK(out.dim() >= 1 && out.size(-1) > 0, "out must be [..., hd]");
  const int hd = (int)out.size(-1);
  TORCH_CHECK(hd % 8 == 0, "row width must be multiple of 8");
  const long rows = out.numel() / hd;
  TORCH_CHECK(in.sizes() == out.sizes(), "in must have out's shape");
  TORCH_CHECK(scales.numel() == rows, "scales must hold one value per row");
  if (rows == 0) return;
  ps_kv_dequant(out.data_ptr(), in.data_ptr(), scales.data_ptr(), rows, hd,
                current_stream());
}

void greedy_sample(at::Tensor out, at::Tensor logits) {
  CHECK_GPU_DTYPE(out, at::kLong);
  CHECK_GPU_BF16(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) > 0,
              "logits must be [R, V], V > 0");
  const long R = logits.size(0);
  const int V = (int)logits.size(1);
  TORCH_CHECK(out.numel() == R, "out must hold one index per row");
  if (R == 0) return;
  ps_greedy_sample(out.data_ptr(), logits.data_ptr(), R, V, current_stream());
}

void resolve_placeholders(at::Tensor tokens, at::Tensor prev_row,
                          at::Tensor prev_tokens) {
  CHECK_GPU_DTYPE(tokens, at::kLong);
  CHECK_GPU_DTYPE(prev_row, at::kInt);
  CHECK_GPU_DTYPE(prev_tokens, at::kLong);
  TORCH_CHECK(tokens.dim() == 1 && prev_row.dim() == 1 &&
                  prev_tokens.dim() == 1,
              "resolve_placeholders takes 1-D tensors");
  TORCH_CHECK(prev_row.numel() == tokens.numel(),
              "prev_row must hold one entry per token row");
  if (tokens.numel() == 0) return;
  int rc = ps_resolve_placeholders(tokens.data_ptr(), prev_row.data_ptr(),
                                   prev_tokens.data_ptr(), tokens.numel(),
                                   prev_tokens.numel(), current_stream());
  TORCH_CHECK(rc == 0, "resolve_placeholders launch rejected");
}

// Python-list front end of ps::step_pack (csrc/step_pack.h). `desc` holds
// five ints per sequence: start, num_tokens, is_decode, sample_last,
// prev_row. `tables` is the list of the sequences' block tables as they are.
// Returns (status, layout fields...) in StepPackLayout order.
py::tuple pack_step_inputs(at::Tensor buf, py::list desc, py::list token_ids,
                           py::list tables, int64_t block_size,
                           int64_t tile_rows) {
  TORCH_CHECK(buf.device().is_cpu() && buf.scalar_type() == at::kByte &&
                  buf.dim() == 1 && buf.is_contiguous(),
              "buf must be a contiguous 1-D uint8 host tensor");
  TORCH_CHECK(block_size > 0 && block_size <= INT32_MAX && tile_rows > 0 &&
                  tile_rows <= INT32_MAX,
              "bad block_size / tile_rows");
  const int64_t n = (int64_t)tables.size();
  TORCH_CHECK((int64_t)desc.size() == 5 * n,
              "desc must hold 5 ints per sequence");
  auto as_long = [](PyObject* o) -> long {
    long v = PyLong_AsLong(o);
    if (v == -1 && PyErr_Occurred()) throw py::error_already_set();
    return v;
  };
  auto as_i32 = [&](PyObject* o) -> int32_t {
    long v = as_long(o);
    TORCH_CHECK(v >= INT32_MIN && v <= INT32_MAX, "value exceeds int32");
    return (int32_t)v;
  };
  std::vector<int32_t> start(n), count(n), prev(n);
  std::vector<uint8_t> dec(n), samp(n);
  std::vector<int64_t> table_off(n + 1, 0);
  for (int64_t s = 0; s < n; ++s) {
    PyObject* d = desc.ptr();
    start[s] = as_i32(PyList_GET_ITEM(d, 5 * s));
    count[s] = as_i32(PyList_GET_ITEM(d, 5 * s + 1));
    dec[s] = as_long(PyList_GET_ITEM(d, 5 * s + 2)) != 0;
    samp[s] = as_long(PyList_GET_ITEM(d, 5 * s + 3)) != 0;
    prev[s] = as_i32(PyList_GET_ITEM(d, 5 * s + 4));
    PyObject* t = PyList_GET_ITEM(tables.ptr(), s);
    TORCH_CHECK(PyList_Check(t), "each block table must be a list");
    table_off[s + 1] = table_off[s] + (int64_t)PyList_GET_SIZE(t);
  }
  std::vector<int32_t> flat(table_off[n]);
  for (int64_t s = 0; s < n; ++s) {
    PyObject* t = PyList_GET_ITEM(tables.ptr(), s);
    int32_t* dst = flat.data() + table_off[s];
    const Py_ssize_t len = PyList_GET_SIZE(t);
    for (Py_ssize_t j = 0; j < len; ++j) {
      dst[j] = as_i32(PyList_GET_ITEM(t, j));
    }
  }
  const int64_t nt = (int64_t)token_ids.size();
  std::vector<int64_t> ids(nt);
  for (int64_t j = 0; j < nt; ++j) {
    ids[j] = as_long(PyList_GET_ITEM(token_ids.ptr(), j));
  }
  ps::StepPackIn in;
  in.num_seqs = n;
  in.start = start.data();
  in.num_tokens = count.data();
  in.is_decode = dec.data();
  in.sample_last = samp.data();
  in.prev_row = prev.data();
  in.token_ids = ids.data();
  in.num_token_ids = nt;
  in.tables = flat.data();
  in.num_table_entries = (int64_t)flat.size();
  in.table_off = table_off.data();
  in.block_size = (int32_t)block_size;
  in.tile_rows = (int32_t)tile_rows;
  ps::StepPackLayout layout;
  const int status =
      ps::step_pack(in, buf.data_ptr(), buf.numel(), &layout);
  py::tuple out(1 + ps::kStepPackFields);
  out[0] = status;
  const int64_t* f = reinterpret_cast<const int64_t*>(&layout);
  for (int64_t i = 0; i < ps::kStepPackFields; ++i) out[1 + i] = f[i];
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rms_norm", &rms_norm, "RMSNorm (bf16)");
  m.def("fused_add_rms_norm", &fused_add_rms_norm,
        "Fused residual add + RMSNorm (bf16, in-place)");
  m.def("silu_and_mul", &silu_and_mul, "SiLU-and-mul (bf16)");
  m.def("rotary_embedding", &rotary_embedding,
        "Neox-style rotary embedding (bf16, in-place)");
  m.def("paged_attn_decode", &paged_attn_decode,
        "Paged attention, decode phase (bf16 KV, split-KV)",
        pybind11::arg("out"), pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("block_tables"),
        pybind11::arg("seq_lens"), pybind11::arg("scale"),
        pybind11::arg("num_splits") = 0, pybind11::arg("variant") = 0,
        pybind11::arg("window") = 0,
        pybind11::arg("order") = pybind11::none());
  m.def("decode_order", &decode_order,
        "Longest-first sequence order for paged_attn_decode");
  m.def("paged_attn_prefill", &paged_attn_prefill,
        "Paged attention, chunked prefill (bf16 KV)");
  m.def("lora_bgmv", &lora_bgmv,
        "batched-grouped LoRA matvec (per-token adapter slots)");
  m.def("paged_attn_prefill_mfma", &paged_attn_prefill_mfma,
        "Paged attention, chunked prefill via MFMA tiles (head_dim 128)",
        pybind11::arg("out"), pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("block_tables"),
        pybind11::arg("tile_info"), pybind11::arg("scale"),
        pybind11::arg("variant") = 4, pybind11::arg("window") = 0);
  m.def("fused_rope_cache", &fused_rope_cache,
        "Fused RoPE + paged KV append on the packed qkv tensor");
  m.def("reshape_and_cache", &reshape_and_cache,
        "Append K/V for new tokens into the paged cache");
  m.def("greedy_sample", &greedy_sample, "Per-row argmax over vocab");
  m.def("resolve_placeholders", &resolve_placeholders,
        "tokens[i] = prev_tokens[prev_row[i]] where prev_row[i] >= 0");
  m.def("pack_step_inputs", &pack_step_inputs,
        "Pack one step's inputs into a host buffer (csrc/step_pack.h)");
  m.def("kv_quant", &kv_quant, "Row-wise int8 KV quantization");
  m.def("rms_norm_fp8", &rms_norm_fp8,
        "RMSNorm (optionally fused residual add) emitting fp8 + row scales");
  m.def("silu_and_mul_fp8", &silu_and_mul_fp8,
        "SiLU-mul emitting fp8 + row scales");
  m.def("cachegen_encode", &cachegen_encode,
        "CacheGen-style adaptive range encode of int8 KV (CPU)");
  m.def("cachegen_decode", &cachegen_decode,
        "CacheGen-style range decode -> int8 (CPU)");
  m.def("gemm8p", &gemm8p,
        "8-phase deep-pipelined bf16 GEMM (out = x @ w.T)");
  m.def("skinny_gemm", &skinny_gemm,
        "Split-K MFMA GEMM for decode-shaped (M<=128) projections");
  m.def("prefill_mfma32_splits", &ps_prefill_mfma32_splits,
        "KV split count paged_attn_prefill_mfma variant 5 runs for (num_tiles, "
        "KH, GQ)",
        pybind11::arg("num_tiles"), pybind11::arg("KH"), pybind11::arg("GQ"));
  m.def("gemm8p_splits", &ps_gemm8p_splits,
        "Split-K depth gemm8p picks for (M, N, K); -1 if unsupported");
  m.def("skinny_gemm_splits", &ps_skinny_gemm_splits,
        "Split-K depth skinny_gemm picks for (M, N, K); -1 if unsupported");
  m.def("skinny_gemm_fp8", &skinny_gemm_fp8,
        "fp8 e4m3 split-K MFMA GEMM with row/channel scales (M<=256)");
  m.def("skinny_gemm_fp8_splits", &ps_skinny_gemm_fp8_splits,
        "Split-K depth skinny_gemm_fp8 picks for (M, N, K); -1 if "
        "unsupported");
  m.def("skinny_gemm_w4", &skinny_gemm_w4,
        "int4 weight-only (group 128) split-K MFMA GEMM, bf16 activations "
        "(M<=256)");
  m.def("skinny_gemm_w4_splits", &ps_skinny_gemm_w4_splits,
        "Split-K depth skinny_gemm_w4 picks for (M, N, K); -1 if "
        "unsupported");
  m.def("int4_dequant", &int4_dequant,
        "Packed int4 + group scales/zero points -> bf16 [N, K]");
  m.def("quant_fp8_rows", &quant_fp8_rows,
        "Per-row fp8 quantization of a (row-strided) bf16 matrix");
  m.def("kv_dequant", &kv_dequant, "Row-wise int8 KV dequantization");
  m.def("fused_moe", &fused_moe,
        "Grouped MoE expert MLP (align + gate_up/SiLU + down + combine)");
  m.def("fused_moe_supported", &fused_moe_supported,
        "Whether fused_moe accepts (T, top_k, E, H, I)");
}
