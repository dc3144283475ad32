"""Pure-PyTorch reference implementations of the HIP kernels.

These serve two purposes:
  1. the fp32 ground truth that every GPU kernel unit test compares against
     (tests/test_kernels_gpu.py);
  2. the CPU execution path, so the whole engine runs (slowly) without a GPU
     for the CPU test tier (fake-engine/CPU tier first).

They intentionally mirror the kernel semantics exactly (paged cache layout
[num_blocks, kv_heads, block_size, head_dim], slot mapping, causal masking).
"""

from __future__ import annotations

import torch


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps) * w.float()
    return out.to(x.dtype)


def fused_add_rms_norm(
    x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float
) -> tuple[torch.Tensor, torch.Tensor]:
    """Returns (normed, new_residual). Matches the in-place kernel: the
    residual accumulator is stored in bf16 (summed in fp32, rounded once).

    This reference norms the ROUNDED (bf16) sum, while the GPU kernels norm
    the fp32 sum they still hold in registers and round only what they store;
    the two differ by up to a bf16 rounding of the norm's input."""
    summed = (x.float() + residual.float()).to(x.dtype)
    return rms_norm(summed, w, eps), summed


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    d = x.shape[-1] // 2
    gate = x[..., :d].float()
    up = x[..., d:].float()
    return (torch.nn.functional.silu(gate) * up).to(x.dtype)


def rotary_embedding(
    positions: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    cos_sin: torch.Tensor,
    head_dim: int,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Neox-style rotation of the leading rot_dim dims of each head.

    q: [T, QH*HD] (or [T, QH, HD]); k analogous. cos_sin: [max_pos, rot_dim]
    laid out as cos[rot/2] || sin[rot/2]. Returns rotated copies.
    """
    T = positions.shape[0]
    rot = cos_sin.shape[-1]
    half = rot // 2
    cs = cos_sin[positions.long()]  # [T, rot]
    cos = cs[:, :half].view(T, 1, half)
    sin = cs[:, half:].view(T, 1, half)

    def rotate(t: torch.Tensor) -> torch.Tensor:
        shape = t.shape
        t = t.view(T, -1, head_dim)
        x1 = t[..., :half].float()
        x2 = t[..., half:rot].float()
        r1 = x1 * cos - x2 * sin
        r2 = x2 * cos + x1 * sin
        out = t.clone()
        out[..., :half] = r1.to(t.dtype)
        out[..., half:rot] = r2.to(t.dtype)
        return out.view(shape)

    return rotate(q), rotate(k)


def reshape_and_cache(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    """k/v: [T, KH, HD]; caches: [NB, KH, BS, HD]; slot_mapping: [T] int64."""
    nb, kh, bs, hd = k_cache.shape
    mask = slot_mapping >= 0
    slots = slot_mapping[mask]
    blk = torch.div(slots, bs, rounding_mode="floor").long()
    off = (slots % bs).long()
    k_cache[blk, :, off] = k.view(-1, kh, hd)[mask].to(k_cache.dtype)
    v_cache[blk, :, off] = v.view(-1, kh, hd)[mask].to(v_cache.dtype)


def _gather_kv(
    cache: torch.Tensor, block_table: torch.Tensor, ctx: int
) -> torch.Tensor:
    """cache: [NB, KH, BS, HD] -> [ctx, KH, HD] for one sequence."""
    nb, kh, bs, hd = cache.shape
    nblocks = (ctx + bs - 1) // bs
    blocks = block_table[:nblocks].long()
    kv = cache[blocks]  # [nblocks, KH, BS, HD]
    kv = kv.permute(0, 2, 1, 3).reshape(nblocks * bs, kh, hd)
    return kv[:ctx]


def paged_attn_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    """q: [S, QH, HD] -> out [S, QH, HD] (fp32 math, cast back).
    window > 0 = sliding-window attention over the last `window` keys."""
    S, QH, HD = q.shape
    KH = k_cache.shape[1]
    GQ = QH // KH
    out = torch.empty_like(q)
    for s in range(S):
        ctx = int(seq_lens[s])
        k = _gather_kv(k_cache, block_tables[s], ctx).float()  # [ctx, KH, HD]
        v = _gather_kv(v_cache, block_tables[s], ctx).float()
        if window and ctx > window:
            k = k[ctx - window:]
            v = v[ctx - window:]
        for h in range(QH):
            kvh = h // GQ
            qs = q[s, h].float()
            logits = (k[:, kvh] @ qs) * scale  # [ctx]
            p = torch.softmax(logits, dim=-1)
            out[s, h] = (p @ v[:, kvh]).to(q.dtype)
    return out


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
    """q: [T, QH, HD]; each token t attends to cache[token_seq[t]][0..pos]
    (or the last `window` positions when window > 0)."""
    T, QH, HD = q.shape
    KH = k_cache.shape[1]
    GQ = QH // KH
    out = torch.empty_like(q)
    for t in range(T):
        s = int(token_seq[t])
        ctx = int(token_pos[t]) + 1
        k = _gather_kv(k_cache, block_tables[s], ctx).float()
        v = _gather_kv(v_cache, block_tables[s], ctx).float()
        if window and ctx > window:
            k = k[ctx - window:]
            v = v[ctx - window:]
        for h in range(QH):
            kvh = h // GQ
            qs = q[t, h].float()
            logits = (k[:, kvh] @ qs) * scale
            p = torch.softmax(logits, dim=-1)
            out[t, h] = (p @ v[:, kvh]).to(q.dtype)
    return out


def greedy_sample(logits: torch.Tensor) -> torch.Tensor:
    return logits.float().argmax(dim=-1)


def resolve_placeholders(
    tokens: torch.Tensor, prev_row: torch.Tensor, prev_tokens: torch.Tensor
) -> torch.Tensor:
    ph = (prev_row >= 0).nonzero().flatten()
    tokens[ph] = prev_tokens[prev_row[ph].long()]
    return tokens


def kv_quant(x: torch.Tensor) -> tuple:
    """Row-wise int8 quantization over the last dim. Returns (int8, scales)."""
    hd = x.shape[-1]
    rows = x.reshape(-1, hd).float()
    amax = rows.abs().amax(dim=-1)
    scales = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.clamp(
        torch.round(rows / scales[:, None]), -127, 127
    ).to(torch.int8)
    return q.view(x.shape), scales


def kv_dequant(q: torch.Tensor, scales: torch.Tensor,
               dtype=torch.bfloat16) -> torch.Tensor:
    hd = q.shape[-1]
    rows = q.reshape(-1, hd).float() * scales[:, None]
    return rows.to(dtype).view(q.shape)


def quant_fp8_rows(x: torch.Tensor) -> tuple:
    """Per-row fp8-e4m3 quantization of [T, D]: scale = max(row amax, 1e-6)
    / 448 (the act-quant kernels' rule). Returns (codes e4m3, scales f32)."""
    xf = x.float()
    scales = xf.abs().amax(dim=-1).clamp(min=1e-6) / 448.0
    q = (xf / scales[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q, scales


def fp8_linear_rowwise(xq, sx, w_q, sw) -> torch.Tensor:
    """out[M, N] bf16 = (xq * sx[:, None]) @ (w_q * sw[:, None]).T as an
    fp32 dequantized matmul: the oracle for the fp8 GEMM kernels."""
    xf = xq.float() * sx.float()[:, None]
    wf = w_q.float() * sw.float()[:, None]
    return (xf @ wf.t()).to(torch.bfloat16)


INT4_GROUP = 128  # k per (scale, zero point) of an int4 weight row


def int4_pack(q: torch.Tensor) -> torch.Tensor:
    """Logical q [N, K] (integers 0..15) -> packed uint8 [N, K/2] in the
    layout csrc/skinny_gemm_w4.hip reads: k = 128c + 32j + 8g + i sits in
    nibble i of the little-endian dword at byte 64c + 16g + 4j of the row."""
    N, K = q.shape
    if K % INT4_GROUP:
        raise ValueError(f"K={K} is not a multiple of {INT4_GROUP}")
    v = q.to(torch.uint8).reshape(N, K // INT4_GROUP, 4, 4, 8)  # c, j, g, i
    v = v.permute(0, 1, 3, 2, 4)  # c, g, j, i
    return (v[..., 0::2] | (v[..., 1::2] << 4)).reshape(N, K // 2)


def int4_unpack(packed: torch.Tensor) -> torch.Tensor:
    """Inverse of int4_pack: packed uint8 [N, K/2] -> q uint8 [N, K]."""
    N, half = packed.shape
    K = half * 2
    if K % INT4_GROUP:
        raise ValueError(f"K={K} is not a multiple of {INT4_GROUP}")
    b = packed.reshape(N, K // INT4_GROUP, 4, 4, 4)  # c, g, j, byte
    v = torch.stack([b & 0xF, b >> 4], dim=-1)  # c, g, j, byte, nibble
    return v.view(N, K // INT4_GROUP, 4, 4, 8).permute(
        0, 1, 3, 2, 4).reshape(N, K)


def int4_quantize_weight(w: torch.Tensor) -> tuple:
    """Round-to-nearest asymmetric int4 with one bf16 scale and one zero
    point per 128 k of a row. Returns (packed uint8 [N, K/2], s bf16
    [N, K/128], z uint8 [N, K/128]). The zero point and the codes are
    computed with the stored (bf16-rounded) scale."""
    N, K = w.shape
    if K % INT4_GROUP:
        raise ValueError(f"K={K} is not a multiple of {INT4_GROUP}")
    g = w.float().view(N, K // INT4_GROUP, INT4_GROUP)
    lo = g.amin(dim=-1).clamp(max=0.0)
    hi = g.amax(dim=-1).clamp(min=0.0)
    s = ((hi - lo).clamp(min=1e-5) / 15.0).to(torch.bfloat16)
    sf = s.float()
    z = torch.round(-lo / sf).clamp(0, 15)
    q = (torch.round(g / sf[..., None]) + z[..., None]).clamp(0, 15)
    return (
        int4_pack(q.to(torch.uint8).view(N, K)), s, z.to(torch.uint8)
    )


def int4_dequant(packed: torch.Tensor, s: torch.Tensor,
                 z: torch.Tensor) -> torch.Tensor:
    """W_deq[n, k] = bf16_rne(float(q[n, k] - z[n, k/128]) * float(s[n,
    k/128])); the fp32 product is exact, the bf16 round is the only one."""
    q = int4_unpack(packed).float()
    zf = z.float().repeat_interleave(INT4_GROUP, dim=1)
    sf = s.float().repeat_interleave(INT4_GROUP, dim=1)
    return ((q - zf) * sf).to(torch.bfloat16)


def int4_linear(x, packed, s, z) -> torch.Tensor:
    """out[M, N] bf16 = x @ W_deq^T with the bf16 W_deq of int4_dequant as
    the operand and fp32 accumulation: the oracle for the int4 GEMM."""
    wd = int4_dequant(packed, s, z)
    return torch.nn.functional.linear(x.float(), wd.float()).to(
        torch.bfloat16)


def lora_bgmv(out, x, A, B, scale, idx, col_off):
    """Reference BGMV: out[t, col_off:+W] += scale[s] * B[s] @ (A[s] @ x[t])
    for s = idx[t] >= 0."""
    import torch

    W = B.shape[1]
    for t in range(x.shape[0]):
        s = int(idx[t])
        if s < 0:
            continue
        y = (A[s].float() @ x[t].float()) * float(scale[s])
        out[t, col_off : col_off + W] += (B[s].float() @ y).to(out.dtype)


def fused_moe(x, experts_gate_up, experts_down, topk_ids, topk_weights):
    """Reference sparse-MoE expert MLP, one (token, k) pair at a time:
    out[t] = sum_k w[t,k] * down_e(silu(gate_e(x[t])) * up_e(x[t])) with
    e = topk_ids[t,k]; fp32 accumulation, the SiLU-mul product rounded to
    the activation dtype where the kernel stores it, k summed in order."""
    import torch

    T, top_k = topk_ids.shape
    inter = experts_down.shape[2]
    xf = x.float()
    wts = topk_weights.float()
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for t in range(T):
        for k in range(top_k):
            e = int(topk_ids[t, k])
            gu = experts_gate_up[e].float() @ xf[t]
            act = torch.nn.functional.silu(gu[:inter]) * gu[inter:]
            act = act.to(x.dtype).float()
            out[t] += wts[t, k] * (experts_down[e].float() @ act)
    return out.to(x.dtype)
