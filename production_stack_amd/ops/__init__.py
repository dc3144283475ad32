"""Op dispatch layer.

On a GPU (any tensor on `cuda`), every op REQUIRES the in-tree HIP extension
production_stack_amd._C and raises if it is missing -- there is no silent
eager fallback on MI355X. On CPU tensors the pure-PyTorch references run so
the engine and its tests work in GPU-less CI.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from production_stack_amd.ops import reference

try:
    from production_stack_amd import _C  # type: ignore[attr-defined]
except ImportError:  # pragma: no cover - exercised only when not built
    _C = None

HAVE_EXT = _C is not None


def _require_ext() -> None:
    if _C is None:
        raise RuntimeError(
            "production_stack_amd._C HIP extension is not built; run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace`. "
            "Refusing to fall back to eager PyTorch on GPU."
        )


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda:
        _require_ext()
        out = torch.empty_like(x)
        _C.rms_norm(out, x, w, eps)
        return out
    return reference.rms_norm(x, w, eps)


def fused_add_rms_norm(
    x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float
) -> tuple[torch.Tensor, torch.Tensor]:
    """In-place on GPU: x <- normed(residual + x); residual <- residual + x."""
    if x.is_cuda:
        _require_ext()
        _C.fused_add_rms_norm(x, residual, w, eps)
        return x, residual
    normed, summed = reference.fused_add_rms_norm(x, residual, w, eps)
    return normed, summed


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        _require_ext()
        d = x.shape[-1] // 2
        out = torch.empty(x.shape[:-1] + (d,), dtype=x.dtype, device=x.device)
        _C.silu_and_mul(out, x)
        return out
    return reference.silu_and_mul(x)


def rotary_embedding(
    positions: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    cos_sin: torch.Tensor,
    head_dim: int,
) -> tuple[torch.Tensor, torch.Tensor]:
    """In-place on GPU. positions int32, q/k bf16 [T, H*HD], cos_sin fp32."""
    if q.is_cuda:
        _require_ext()
        _C.rotary_embedding(positions, q, k, cos_sin, head_dim)
        return q, k
    return reference.rotary_embedding(positions, q, k, cos_sin, head_dim)


def fused_rope_cache(
    qkv: torch.Tensor,
    positions: torch.Tensor,
    cos_sin: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    q_heads: int,
    head_dim: int,
) -> None:
    """Fused in-place RoPE on packed qkv + paged KV append (GPU only)."""
    _require_ext()
    _C.fused_rope_cache(
        qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, q_heads,
        head_dim,
    )


def reshape_and_cache(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    if k_cache.is_cuda:
        _require_ext()
        _C.reshape_and_cache(
            k.view(k.shape[0], -1), v.view(v.shape[0], -1), k_cache, v_cache,
            slot_mapping,
        )
        return
    reference.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


# Decode attention kernel variant (csrc/attention.hip): 3 = the low-register
# packed-q kernel with the next block's K tile and the block-table entry two
# blocks ahead prefetched and the score reduction in DPP instead of LDS
# shuffles; bit-identical to variants 1 and 2, 2% faster than variant 2 at
# the flagship ragged shape and 8% where the batch shares a cached prompt
# prefix (profiles/README.md). An fp8 KV cache runs variant 2 = variant 1
# with the next block-table entry prefetched. PS_DECODE_VARIANT=2 (or 1)
# restores those for A/B.
DECODE_VARIANT = int(os.environ.get("PS_DECODE_VARIANT", "3"))
# Longest-first launch order for decode attention (decode_order), computed
# by the model once per forward; PS_DECODE_ORDER=0 turns it off for A/B.
DECODE_ORDER = os.environ.get("PS_DECODE_ORDER", "1") != "0"


def _check_out(out: torch.Tensor, q: torch.Tensor) -> None:
    """An attention `out=` buffer is written as dense [T, QH, HD] rows."""
    if (
        out.shape != q.shape
        or out.dtype != q.dtype
        or out.device != q.device
        or not out.is_contiguous()
    ):
        raise ValueError(
            "out must be contiguous with q's shape, dtype and device"
        )


def paged_attn_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float,
    window: int = 0,
    order: Optional[torch.Tensor] = None,
    out: Optional[torch.Tensor] = None,
    variant: Optional[int] = None,
) -> torch.Tensor:
    """`order` (see decode_order) only changes the order in which the GPU
    kernel's workgroups are launched, never a result; the CPU reference
    ignores it. `out` (contiguous, q's shape and dtype) receives the result
    and is returned; `variant` overrides DECODE_VARIANT for this call."""
    if out is not None:
        _check_out(out, q)
    if q.is_cuda:
        _require_ext()
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        # variants 1-3 = low-register packed-q kernel (3 waves/SIMD):
        # measured +17-26% over variant 0 across batch/ctx
        # (profiles/attn_bench).
        _C.paged_attn_decode(
            out, q, k_cache, v_cache, block_tables, seq_lens, scale, 0,
            DECODE_VARIANT if variant is None else variant, window, order
        )
        return out
    res = reference.paged_attn_decode(
        q, k_cache, v_cache, block_tables, seq_lens, scale, window
    )
    if out is None:
        return res
    out.copy_(res)
    return out


def decode_order(seq_lens: torch.Tensor) -> Optional[torch.Tensor]:
    """Indices of `seq_lens` (int32 [S]) sorted longest first, ties by
    ascending index (a stable descending argsort), as int32 [S]: the launch
    order for paged_attn_decode, so that a ragged batch starts its long
    sequences first and the launch drains evenly. On the GPU one small
    kernel with no host sync (hipGraph-safe); returns None when S is more
    than that kernel handles, and the caller then passes no order."""
    if seq_lens.is_cuda:
        _require_ext()
        order = torch.empty_like(seq_lens)
        if not _C.decode_order(order, seq_lens):
            return None
        return order
    return torch.argsort(-seq_lens, stable=True).int()


def paged_attn_prefill(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    token_seq: torch.Tensor,
    token_pos: torch.Tensor,
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    if q.is_cuda:
        _require_ext()
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _C.paged_attn_prefill(
            out, q, k_cache, v_cache, block_tables, token_seq, token_pos,
            scale, window
        )
        return out
    return reference.paged_attn_prefill(
        q, k_cache, v_cache, block_tables, token_seq, token_pos, scale,
        window
    )


# Default MFMA prefill variant: 5 = 8-wave 32x32 swapped-QK^T kernel
# (csrc/prefill_mfma32.hip); 3/4 = the 4-wave 16x16 kernel (64-row
# tiles). Overridable for A/B via PS_PREFILL_VARIANT.
PREFILL_VARIANT = int(os.environ.get("PS_PREFILL_VARIANT", "5"))


def prefill_tile_rows(num_q_heads: int, num_kv_heads: int) -> int:
    """Prefill tile row count for the active kernel. v5 splits its 8 waves
    into GQW head-columns x row-halves (GQW = largest pow2 divisor of the
    GQA ratio, <=4), so tiles carry 32*(8/GQW) rows (64..256)."""
    if PREFILL_VARIANT != 5:
        return 64
    gq = max(1, num_q_heads // max(1, num_kv_heads))
    gqw = 1
    while gqw < 4 and gq % (gqw * 2) == 0:
        gqw *= 2
    return 32 * (8 // gqw)


def paged_attn_prefill_mfma(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    tile_info: torch.Tensor,
    scale: float,
    window: int = 0,
    variant: int = None,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """MFMA-tiled chunked prefill (GPU, head_dim 128 only). tile_info rows
    must be built with n_rows <= prefill_tile_rows() for the active
    variant. `out` (contiguous, q's shape and dtype) receives the result.

    Precondition: every row of q belongs to exactly one tile. Variant 5's
    split-KV merge writes all q.shape[0] rows of `out` from per-row
    partials that only a tile's workgroups fill in, so a row that no tile
    covers would be merged from uninitialised workspace. q may be a row
    slice of a wider buffer (stride(0) is free; heads must be packed)."""
    _require_ext()
    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    else:
        _check_out(out, q)
    # v5's split-KV (up to 8 kv-splits) keeps CUs filled at small
    # serving launches, where it now beats v3 at the canonical shapes
    # (12-seq x 200-row continuation at hist 4600: 305 vs 263 TF; fresh
    # 900-row prefill: 400 vs 306) as well as at large ones — so v5 is
    # the default everywhere (PS_PREFILL_VARIANT=3 restores the 4-wave
    # kernel for A/B).
    v = PREFILL_VARIANT if variant is None else variant
    _C.paged_attn_prefill_mfma(
        out, q, k_cache, v_cache, block_tables, tile_info, scale, v, window
    )
    return out


def greedy_sample(logits: torch.Tensor) -> torch.Tensor:
    if logits.is_cuda:
        _require_ext()
        if logits.dtype != torch.bfloat16:  # penalty-adjusted fp32 rows
            return logits.float().argmax(dim=-1)
        out = torch.empty(
            logits.shape[0], dtype=torch.long, device=logits.device
        )
        _C.greedy_sample(out, logits)
        return out
    return reference.greedy_sample(logits)


def resolve_placeholders(
    tokens: torch.Tensor, prev_row: torch.Tensor, prev_tokens: torch.Tensor
) -> torch.Tensor:
    """In place: tokens[i] = prev_tokens[prev_row[i]] where prev_row[i] >= 0
    (async scheduling: rows whose input token the previous step is still
    sampling). tokens/prev_tokens int64, prev_row int32, one per row."""
    if tokens.is_cuda:
        _require_ext()
        _C.resolve_placeholders(tokens, prev_row, prev_tokens)
        return tokens
    return reference.resolve_placeholders(tokens, prev_row, prev_tokens)


# status codes of pack_step_inputs (csrc/step_pack.h)
PACK_OK = 0
PACK_TOO_SMALL = 1
PACK_PREFILL_PLACEHOLDER = 2
PACK_DECODE_UNRESOLVED = 3
PACK_BAD_INPUT = 4

# StepPackLayout fields, in order, after the status
PACK_FIELDS = (
    "total_bytes", "num_tokens", "num_prefill_tokens", "num_prefill_seqs",
    "num_decode_seqs", "num_tiles", "max_bt", "num_sample_rows",
    "num_placeholders", "off_tokens", "off_positions", "off_slot_mapping",
    "off_prefill_token_seq", "off_prefill_token_pos", "off_prefill_tiles",
    "off_prefill_block_tables", "off_decode_block_tables",
    "off_decode_seq_lens", "off_sample_rows", "off_prev_row",
)


def pack_step_inputs(
    buf: torch.Tensor,
    desc: list,
    token_ids: list,
    tables: list,
    block_size: int,
    tile_rows: int,
) -> tuple:
    """Pack one step's inputs into the uint8 host tensor `buf` (host-only
    C++, csrc/step_pack.h). `desc` holds five ints per sequence (start,
    num_tokens, is_decode, sample_last, prev_row), `token_ids` the chunks'
    ids back to back, `tables` the block tables as they are. Returns
    (status, layout dict); nothing is written unless status is PACK_OK."""
    _require_ext()
    res = _C.pack_step_inputs(
        buf, desc, token_ids, tables, block_size, tile_rows
    )
    return res[0], dict(zip(PACK_FIELDS, res[1:]))


def kv_quant(x: torch.Tensor) -> tuple:
    """Row-wise int8 KV quantization (CacheGen-style serde)."""
    if x.is_cuda:
        _require_ext()
        hd = x.shape[-1]
        out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
        scales = torch.empty(
            x.numel() // hd, dtype=torch.float32, device=x.device
        )
        _C.kv_quant(out, scales, x)
        return out, scales
    return reference.kv_quant(x)


def kv_dequant(
    q: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16
) -> torch.Tensor:
    if q.is_cuda:
        _require_ext()
        out = torch.empty(q.shape, dtype=dtype, device=q.device)
        _C.kv_dequant(out, q, scales)
        return out
    return reference.kv_dequant(q, scales, dtype)


def skinny_gemm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """out = x @ w.T for decode-shaped 1 <= M <= 256, N and K multiples of
    64 (weight-stream-bound GEMMs where hipBLASLt tiles poorly — see
    csrc/skinny_gemm.hip). GPU only."""
    _require_ext()
    out = torch.empty(
        (x.shape[0], w.shape[0]), dtype=torch.bfloat16, device=x.device
    )
    _C.skinny_gemm(out, x, w)  # split-K partials + combine (no atomics)
    return out


def cachegen_encode(q: torch.Tensor) -> torch.Tensor:
    """Entropy-encode int8 KV (CPU adaptive range coder, per-channel
    contexts). Falls back to a pure-Python reference when the extension
    is unavailable (CPU CI)."""
    if _C is not None and hasattr(_C, "cachegen_encode"):
        return _C.cachegen_encode(q.contiguous().cpu())
    return reference.cachegen_encode(q)


def cachegen_decode(blob: torch.Tensor, hd: int) -> torch.Tensor:
    if _C is not None and hasattr(_C, "cachegen_decode"):
        return _C.cachegen_decode(blob.contiguous().cpu(), hd)
    return reference.cachegen_decode(blob, hd)


def gemm8p(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """out = x @ w.T via the 8-phase deep-pipelined MFMA GEMM
    (csrc/gemm8p.hip; 256x256 tiles + split-K for skinny M). GPU only."""
    _require_ext()
    out = torch.empty(
        (x.shape[0], w.shape[0]), dtype=torch.bfloat16, device=x.device
    )
    _C.gemm8p(out, x, w)
    return out


def lora_bgmv(
    out: torch.Tensor,
    x: torch.Tensor,
    A: torch.Tensor,
    B: torch.Tensor,
    scale: torch.Tensor,
    idx: torch.Tensor,
    col_off: int = 0,
) -> None:
    """out[t, col_off:+W] += scale[idx[t]] * B[idx[t]] @ (A[idx[t]] @ x[t]);
    idx[t] < 0 skips the row. hipGraph-safe (static shapes, no host sync)."""
    if out.is_cuda:
        _require_ext()
        _C.lora_bgmv(out, x, A, B, scale, idx, col_off)
        return
    reference.lora_bgmv(out, x, A, B, scale, idx, col_off)


FUSED_MOE_MAX_PAIRS = 1024  # T * top_k, one moe_align workgroup
FUSED_MOE_MAX_EXPERTS = 64


def fused_moe_supported(T: int, top_k: int, E: int, H: int, I: int) -> bool:
    """The accept rule of csrc/moe_fused.hip (ps_fused_moe_supported):
    decode-sized batches, 64-aligned hidden/intermediate widths."""
    return (
        T >= 1 and 1 <= top_k <= E <= FUSED_MOE_MAX_EXPERTS
        and T * top_k <= FUSED_MOE_MAX_PAIRS
        and H >= 64 and I >= 64 and H % 64 == 0 and I % 64 == 0
    )


def fused_moe(
    x: torch.Tensor,
    experts_gate_up: torch.Tensor,
    experts_down: torch.Tensor,
    topk_ids: torch.Tensor,
    topk_weights: torch.Tensor,
) -> torch.Tensor:
    """Sparse-MoE expert MLP for routed tokens: x [T, H] bf16, gate_up
    [E, 2I, H], down [E, H, I], topk_ids/topk_weights [T, top_k] ->
    [T, H] bf16. On the GPU the launch sequence depends only on the shapes
    (no host sync, no atomics): hipGraph-safe and bit-deterministic.
    Unsupported shapes raise (see fused_moe_supported)."""
    if x.is_cuda:
        _require_ext()
        T, H = x.shape
        top_k = topk_ids.shape[1]
        E, _, I = experts_down.shape
        P = T * top_k
        dev = x.device
        # scratch via torch.empty so it lands in the graph pool under
        # capture; the kernels overwrite every element they later read
        out = torch.empty((T, H), dtype=torch.bfloat16, device=dev)
        offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
        sorted_pairs = torch.empty(P, dtype=torch.int32, device=dev)
        act = torch.empty((P, I), dtype=torch.bfloat16, device=dev)
        y = torch.empty((P, H), dtype=torch.float32, device=dev)
        _C.fused_moe(
            out, offsets, sorted_pairs, act, y, x, experts_gate_up,
            experts_down, topk_ids.contiguous(),
            topk_weights.float().contiguous(),
        )
        return out
    return reference.fused_moe(
        x, experts_gate_up, experts_down, topk_ids, topk_weights
    )


def fp8_linear(
    x: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor
) -> torch.Tensor:
    """out = x @ (w_q * w_scale)^T with fp8 tensor cores.

    Weights are stored OCP fp8-e4m3 with a per-tensor scale; activations
    quantize dynamically per call (per-tensor amax / 448). On gfx950 this
    runs through hipBLASLt's fp8 MFMA path (torch._scaled_mm) at ~1.8x
    the bf16 GEMM rate for decode shapes. CPU fallback dequantizes.
    """
    if x.is_cuda:
        sx = (x.abs().amax().clamp(min=1e-6) / 448.0).to(torch.float32)
        xq = (x / sx).to(torch.float8_e4m3fn)
        if w_scale.dim() == 1:  # per-channel weight scales
            return fp8_linear_rowwise(
                xq, sx.expand(x.shape[0]), w_q, w_scale)
        return torch._scaled_mm(
            xq, w_q.t(), scale_a=sx, scale_b=w_scale,
            out_dtype=torch.bfloat16,
        )
    wf = w_q.float() * (
        w_scale.float()[:, None] if w_scale.dim() == 1
        else w_scale.float()
    )
    return torch.nn.functional.linear(x.float(), wf).to(x.dtype)


def fp8_quantize_weight(w: torch.Tensor):
    """Per-tensor weight quantization: returns (w_q fp8, scale f32)."""
    scale = (w.abs().amax().float().clamp(min=1e-6) / 448.0)
    w_q = (w.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
    return w_q, scale


def fp8_quantize_weight_rowwise(w: torch.Tensor):
    """Per-output-channel weight quantization: (w_q fp8 [N,K], scales
    [N] f32) — finer than per-tensor, same GEMM cost with rowwise-scaled
    fp8 matmul."""
    scales = (w.abs().amax(dim=1).float().clamp(min=1e-6) / 448.0)
    w_q = (w.float() / scales[:, None]).clamp(-448, 448).to(
        torch.float8_e4m3fn)
    return w_q, scales


def rms_norm_fp8(x, w, eps, residual=None):
    """Fused (add-)RMSNorm emitting fp8-e4m3 rows + per-row scales. When
    `residual` is given it is updated in place (residual += x) like
    fused_add_rms_norm. GPU only."""
    _require_ext()
    T, D = x.shape
    out_q = torch.empty((T, D), dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty(T, dtype=torch.float32, device=x.device)
    _C.rms_norm_fp8(out_q, scales, x,
                    residual if residual is not None else x, w, eps,
                    1 if residual is not None else 0)
    return out_q, scales


def silu_and_mul_fp8(x):
    _require_ext()
    T, D2 = x.shape
    out_q = torch.empty((T, D2 // 2), dtype=torch.float8_e4m3fn,
                        device=x.device)
    scales = torch.empty(T, dtype=torch.float32, device=x.device)
    _C.silu_and_mul_fp8(out_q, scales, x)
    return out_q, scales


_ROWWISE_SCALED_MM = None  # probed once: does _scaled_mm accept [M,1]x[1,N]?


def fp8_rowwise_supported(device="cuda") -> bool:
    """Whether this build's _scaled_mm takes rowwise scales. When it does
    not, the fused per-row act-quant path would need a slow fp32-out
    fallback, so callers keep the per-tensor fp8 pipeline instead."""
    global _ROWWISE_SCALED_MM
    if _ROWWISE_SCALED_MM is None:
        try:
            torch._scaled_mm(
                torch.zeros(16, 32, dtype=torch.float8_e4m3fn,
                            device=device),
                torch.zeros(32, 16, dtype=torch.float8_e4m3fn,
                            device=device),
                scale_a=torch.ones(16, 1, device=device),
                scale_b=torch.ones(1, 16, device=device),
                out_dtype=torch.bfloat16,
            )
            _ROWWISE_SCALED_MM = True
        except (RuntimeError, TypeError):
            _ROWWISE_SCALED_MM = False
    return _ROWWISE_SCALED_MM


def skinny_gemm_fp8_supported(M: int, N: int, K: int) -> bool:
    """The accept rule of csrc/skinny_gemm_fp8.hip
    (ps_skinny_gemm_fp8_splits > 0): decode-sized M, 64-aligned N and K."""
    return (
        1 <= M <= 256 and N >= 64 and K >= 64
        and N % 64 == 0 and K % 64 == 0
    )


def skinny_gemm_fp8(xq, sx, wq, sw) -> torch.Tensor:
    """out[M,N] bf16 = (xq*sx[:,None]) @ (wq*sw[:,None]).T with xq [M,K]
    and wq [N,K] OCP e4m3, sx [M] and sw [N] fp32, through the hand-written
    fp8 MFMA kernel (csrc/skinny_gemm_fp8.hip): fp32 accumulation, scales
    applied once before the bf16 round, bit-deterministic, and a row's
    result does not depend on M. GPU only; shapes outside
    skinny_gemm_fp8_supported raise. M == 0 returns an empty [0, N]."""
    _require_ext()
    out = torch.empty(
        (xq.shape[0], wq.shape[0]), dtype=torch.bfloat16, device=xq.device
    )
    if xq.shape[0] == 0:
        return out
    _C.skinny_gemm_fp8(out, xq, sx, wq, sw)
    return out


def quant_fp8_rows(x: torch.Tensor):
    """Per-row dynamic fp8 quantization of a bf16 [T, D] matrix (rows may
    be strided): returns (xq e4m3 [T, D], sx fp32 [T]) with
    sx = max(row amax, 1e-6) / 448, the rule of the fused act-quant
    kernels. x is left unchanged."""
    if x.is_cuda:
        _require_ext()
        T, D = x.shape
        out_q = torch.empty((T, D), dtype=torch.float8_e4m3fn,
                            device=x.device)
        scales = torch.empty(T, dtype=torch.float32, device=x.device)
        _C.quant_fp8_rows(out_q, scales, x)
        return out_q, scales
    return reference.quant_fp8_rows(x)


def fp8_linear_rowwise(xq, sx, w_q, sw, backend="scaled_mm"):
    """out[M,N] = (xq*sx[:,None]) @ (w_q*sw[None,:]).T in fp8 tensor
    cores with per-row activation + per-channel weight scales. Uses
    _scaled_mm's rowwise scaling when this build supports it, else a
    unit-scale fp8 GEMM with the outer-product scale applied after.

    backend="native" runs skinny_gemm_fp8 instead when the input is on the
    GPU and skinny_gemm_fp8_supported(M, N, K) holds. Everything else
    (prefill chunks with M > 256, shard shapes that are not 64-aligned)
    falls through to the _scaled_mm path above, unchanged."""
    if backend not in ("scaled_mm", "native"):
        raise ValueError(
            f"unknown fp8 gemm backend {backend!r}; "
            "expected 'scaled_mm' or 'native'"
        )
    if (
        backend == "native" and xq.is_cuda
        and skinny_gemm_fp8_supported(xq.shape[0], w_q.shape[0], xq.shape[1])
    ):
        return skinny_gemm_fp8(xq, sx, w_q, sw)
    if fp8_rowwise_supported(xq.device):
        return torch._scaled_mm(
            xq, w_q.t(), scale_a=sx[:, None].contiguous(),
            scale_b=sw[None, :].contiguous(), out_dtype=torch.bfloat16,
        )
    one = torch.ones((), dtype=torch.float32, device=xq.device)
    out = torch._scaled_mm(xq, w_q.t(), scale_a=one, scale_b=one,
                           out_dtype=torch.float32)
    return (out * sx[:, None] * sw[None, :]).to(torch.bfloat16)


# ---- int4 weight-only quantization (W4A16, group 128) ----
# W_deq[n, k] = bf16_rne(float(q[n, k] - z[n, k/128]) * float(s[n, k/128]));
# every path multiplies x by these bf16 values with fp32 accumulation.

INT4_GROUP = reference.INT4_GROUP

# The nibble order belongs to csrc/skinny_gemm_w4.hip; these two and the
# kernels are the only code that knows it. Both take CPU and GPU tensors.
int4_pack = reference.int4_pack
int4_unpack = reference.int4_unpack


def int4_quantize_weight(w: torch.Tensor):
    """Round-to-nearest asymmetric int4 of w [N, K] with one bf16 scale and
    one zero point per 128 k of a row: (packed uint8 [N, K/2], s bf16
    [N, K/128], z uint8 [N, K/128]), on w's device."""
    return reference.int4_quantize_weight(w)


def int4_dequant(packed, s, z) -> torch.Tensor:
    """packed + s + z -> W_deq [N, K] bf16 (csrc/skinny_gemm_w4.hip on the
    GPU, the reference formula on the CPU)."""
    if packed.is_cuda:
        _require_ext()
        out = torch.empty(
            (packed.shape[0], packed.shape[1] * 2), dtype=torch.bfloat16,
            device=packed.device,
        )
        _C.int4_dequant(out, packed, s, z)
        return out
    return reference.int4_dequant(packed, s, z)


def skinny_gemm_w4_supported(M: int, N: int, K: int) -> bool:
    """The accept rule of csrc/skinny_gemm_w4.hip
    (ps_skinny_gemm_w4_splits > 0): decode-sized M, 64-aligned N, K in whole
    128-wide quantization groups."""
    return (
        1 <= M <= 256 and N >= 64 and K >= INT4_GROUP
        and N % 64 == 0 and K % INT4_GROUP == 0
    )


def skinny_gemm_w4(x, packed, s, z) -> torch.Tensor:
    """out[M,N] bf16 = x[M,K] bf16 @ W_deq[N,K]^T through the hand-written
    int4 MFMA kernel (csrc/skinny_gemm_w4.hip): weights dequantized in
    registers to the bf16 values of int4_dequant, fp32 accumulation,
    bit-deterministic, and a row's result does not depend on M. GPU only;
    shapes outside skinny_gemm_w4_supported raise. M == 0 returns an empty
    [0, N]."""
    _require_ext()
    out = torch.empty(
        (x.shape[0], packed.shape[0]), dtype=torch.bfloat16, device=x.device
    )
    if x.shape[0] == 0:
        return out
    _C.skinny_gemm_w4(out, x, packed, s, z)
    return out


def int4_linear(x, packed, s, z) -> torch.Tensor:
    """x @ W_deq^T for an int4 weight: the native kernel when x is on the
    GPU and skinny_gemm_w4_supported(M, N, K) holds; otherwise (prefill
    chunks with M > 256) int4_dequant into a transient bf16 buffer and the
    bf16 GEMM dispatch; the reference on the CPU."""
    if not x.is_cuda:
        return reference.int4_linear(x, packed, s, z)
    if skinny_gemm_w4_supported(x.shape[0], packed.shape[0], x.shape[1]):
        return skinny_gemm_w4(x, packed, s, z)
    from production_stack_amd.ops import gemm_policy

    return gemm_policy.linear(x, int4_dequant(packed, s, z))
