"""fp64 references and pass criteria for the norm / activation / RoPE /
quantization / LoRA / sampling kernels.

Everything here is plain torch on the CPU, computed in float64 from the bf16
inputs, and independent of production_stack_amd.ops.reference and of any GPU
kernel. tests/test_elementwise_criteria_cpu.py shows that each criterion
accepts an honest fp32 evaluation of its op and rejects subtly wrong ones;
tests/test_elementwise_edges_gpu.py applies the same criteria to the kernels.

A criterion raises AssertionError and otherwise returns its worst figure (in
units of its own bound), so a caller can print it.
"""

from __future__ import annotations

import torch

F64 = torch.float64
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn

# The kernels evaluate in fp32 what the references evaluate in fp64. One
# percent of a half-step is >= 2^-9 * 0.01 = 2e-5 relative for bf16 and
# >= 2^-5 * 0.01 = 3e-4 relative for e4m3, against about 1e-5 of fp32 noise
# (a few roundings at 2^-24 each, a tree sum of D squares, __expf).
MARGIN = 1.01


def _cpu64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().to(F64)


def _floor_log2(a: torch.Tensor) -> torch.Tensor:
    """floor(log2|a|) from the float64 exponent field; 0 maps to -1075."""
    _, e = torch.frexp(a.abs())  # |a| = m * 2^e, m in [0.5, 1)
    e = e.to(torch.int64) - 1
    return torch.where(a == 0, torch.full_like(e, -1075), e)


# ---------------------------------------------------------------------------
# bf16: one rounding from a higher-precision value
# ---------------------------------------------------------------------------
def half_ulp_bf16(ref64: torch.Tensor) -> torch.Tensor:
    """Half the bf16 spacing at ref: 2^(floor(log2|ref|) - 8), the exponent
    clamped at -126 (subnormals, and 0, sit on the 2^-133 grid)."""
    e = _floor_log2(ref64).clamp(min=-126)
    return torch.ldexp(torch.ones_like(ref64), e - 8)


def assert_bf16_rounded(got, ref64, slack=0.0, what="") -> float:
    """|got - ref| <= half_ulp_bf16(ref) * 1.01 + slack, elementwise. `slack`
    (a number or a tensor like ref) is the absolute error the op may carry
    before its final rounding; 0 for O(1) fp32 operations per element."""
    assert got.dtype == BF16, got.dtype
    g = _cpu64(got)
    r = _cpu64(ref64)
    assert g.shape == r.shape, (g.shape, r.shape)
    assert torch.isfinite(r).all(), "reference must be finite"
    bound = half_ulp_bf16(r) * MARGIN + torch.as_tensor(slack, dtype=F64)
    err = (g - r).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    bad = err > bound
    worst = float((err / bound).max()) if err.numel() else 0.0
    if bad.any():
        i = int((err / bound).flatten().argmax())
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} elements beyond one bf16 "
            f"rounding; worst {worst:.3f}x the bound at flat index {i}: "
            f"got {float(g.flatten()[i])!r} ref {float(r.flatten()[i])!r}"
        )
    return worst


def assert_bits_equal(got, want, what="") -> None:
    """Same dtype, same shape, same bytes (so -0 != +0 and NaNs compare)."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    a = got.view(torch.uint8)
    b = want.view(torch.uint8)
    if not torch.equal(a, b):
        n = int((a != b).sum())
        raise AssertionError(f"{what}: {n} bytes differ")


# ---------------------------------------------------------------------------
# fp8 e4m3 rows with a per-row scale
# ---------------------------------------------------------------------------
FP8_MAX = 448.0
FP8_AMAX_FLOOR = 1e-6  # the kernels start the row amax from this


def half_step_e4m3(r64: torch.Tensor) -> torch.Tensor:
    """Half the e4m3 spacing at r: 2^(floor(log2|r|) - 4), the exponent
    clamped to [-6, 8] (subnormal step 2^-9; top binade [256, 448])."""
    e = _floor_log2(r64).clamp(min=-6, max=8)
    return torch.ldexp(torch.ones_like(r64), e - 4)


def _fp8_codes_to_f64(codes: torch.Tensor) -> torch.Tensor:
    c = codes.detach().cpu()
    if c.dtype == torch.uint8:
        c = c.view(FP8)
    assert c.dtype == FP8, c.dtype
    return c.to(torch.float32).to(F64)


def assert_fp8_rounded(codes, scale_got, ref64, what="") -> float:
    """codes [T, D] (e4m3), scale_got [T] fp32 (None: unit scale, no scale
    check), ref64 [T, D]. With r = ref / scale_got[:, None]:
    |float(codes) - r| <= half_step_e4m3(r) * 1.01, and scale_got within
    rtol 1e-5 of max(amax|ref|, 1e-6) / 448. An all-zero row therefore has
    scale 1e-6/448 and all codes 0."""
    r = _cpu64(ref64)
    q = _fp8_codes_to_f64(codes)
    assert q.shape == r.shape, (q.shape, r.shape)
    assert torch.isfinite(q).all(), f"{what}: non-finite fp8 code"
    if scale_got is not None:
        s = _cpu64(scale_got)
        assert s.shape == (r.shape[0],), s.shape
        want = r.abs().amax(dim=1).clamp(min=FP8_AMAX_FLOOR) / FP8_MAX
        rel = ((s - want).abs() / want).max()
        assert float(rel) <= 1e-5, (
            f"{what}: row scale off by {float(rel):.3e} relative "
            f"(got {s.tolist()[:4]}, want {want.tolist()[:4]})"
        )
        zero_rows = r.abs().amax(dim=1) == 0
        assert (q[zero_rows] == 0).all(), f"{what}: zero row has non-zero codes"
        r = r / s[:, None]
    bound = half_step_e4m3(r) * MARGIN
    err = (q - r).abs()
    worst = float((err / bound).max()) if err.numel() else 0.0
    bad = err > bound
    if bad.any():
        i = int((err / bound).flatten().argmax())
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} codes beyond one e4m3 "
            f"rounding; worst {worst:.3f}x at flat index {i}: "
            f"code {float(q.flatten()[i])!r} for r={float(r.flatten()[i])!r}"
        )
    return worst


# ---------------------------------------------------------------------------
# int8 rows with a per-row scale (kv_quant)
# ---------------------------------------------------------------------------
def assert_int8_codes(q_got, s_got, x, what="") -> int:
    """Scales within rtol 1e-6 of fp64 amax/127 (1.0 for a zero row); codes
    equal round_half_even(x64 / scale64) except where the quotient's
    fractional part is within 1e-4 of 0.5, where +-1 is allowed (the fp32
    quotient x * (1/scale) carries up to 127 * 2^-22 = 3e-5 of error, which
    can push a near-tie either way). Returns the number of such mismatches."""
    x64 = _cpu64(x).reshape(-1, x.shape[-1])
    q = q_got.detach().cpu().reshape(x64.shape)
    assert q.dtype == torch.int8, q.dtype
    s = _cpu64(s_got).reshape(-1)
    assert s.shape[0] == x64.shape[0], (s.shape, x64.shape)
    amax = x64.abs().amax(dim=1)
    s64 = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    rel = ((s - s64).abs() / s64).max()
    assert float(rel) <= 1e-6, f"{what}: scale off by {float(rel):.3e} relative"
    quo = x64 / s64[:, None]
    want = torch.round(quo).clamp(-127, 127)  # torch.round is half-to-even
    diff = q.to(F64) - want
    frac = (quo - torch.floor(quo) - 0.5).abs()
    # A row whose scale is a power of two (amax = 127 * 2^m, or a zero row)
    # has an exact 1/scale and exact quotients in fp32 as in fp64, so its
    # ties are true ties and must go to even: no allowance there. This is
    # what tells round-half-even from round-half-away.
    inexact = (torch.frexp(s64)[0] != 0.5)[:, None]
    tie = (frac <= 1e-4) & inexact
    bad =(diff != 0) & ~(tie & (diff.abs() == 1))
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} wrong int8 codes, first at flat index "
            f"{i}: got {int(q.flatten()[i])} for quotient "
            f"{float(quo.flatten()[i])!r}"
        )
    return int((diff != 0).sum())


# ---------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------
def ref_rms_norm(x, w, eps, residual=None) -> torch.Tensor:
    """x * rsqrt(mean(x^2) + eps) * w in fp64. With `residual`, the row that
    is normed is x + residual before any rounding, as the kernels do it."""
    v = _cpu64(x)
    if residual is not None:
        v = v + _cpu64(residual)
    inv = torch.rsqrt((v * v).mean(dim=-1, keepdim=True) + eps)
    return v * inv * _cpu64(w)


def residual_sum_bf16(x, residual) -> torch.Tensor:
    """The updated residual: summed in fp32, rounded once to bf16."""
    return (x.detach().cpu().float() + residual.detach().cpu().float()).to(BF16)


def ref_silu_and_mul(x) -> torch.Tensor:
    v = _cpu64(x)
    d = v.shape[-1] // 2
    g, u = v[..., :d], v[..., d:]
    return g / (1.0 + torch.exp(-g)) * u


def rope_table(max_pos: int, rot: int, theta: float = 500000.0) -> torch.Tensor:
    """[max_pos, rot] fp32: cos[rot/2] || sin[rot/2], the layout the kernels
    read."""
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=F64) / rot))
    ang = torch.outer(torch.arange(max_pos, dtype=F64), inv)
    return torch.cat([ang.cos(), ang.sin()], dim=-1).float().contiguous()


def ref_rope(positions, heads, cos_sin, hd):
    """Neox-style rotation of the leading `rot` dims of every head.
    heads: [T, H*hd] bf16. Returns (ref64 [T, H*hd], slack [T, H*hd]).

    The two products of x1*c - x2*s can cancel, so the fp32 evaluation carries
    an absolute error that does not shrink with the result. Each product and
    the sum round at 2^-24 relative (a fused multiply-add only drops one of
    them), hence slack = 2^-23 * (|x1*c| + |x2*s|); dims past `rot` get 0.
    """
    T = heads.shape[0]
    v = _cpu64(heads).reshape(T, -1, hd)
    cs = _cpu64(cos_sin)[positions.detach().cpu().long()]  # [T, rot]
    rot = cs.shape[1]
    half = rot // 2
    c = cs[:, None, :half]
    s = cs[:, None, half:]
    x1, x2 = v[..., :half], v[..., half:rot]
    out = v.clone()
    out[..., :half] = x1 * c - x2 * s
    out[..., half:rot] = x2 * c + x1 * s
    slack = torch.zeros_like(v)
    slack[..., :half] = (x1 * c).abs() + (x2 * s).abs()
    slack[..., half:rot] = (x2 * c).abs() + (x1 * s).abs()
    slack *= 2.0 ** -23
    return out.reshape(T, -1), slack.reshape(T, -1)


def check_rope(got, before, positions, cos_sin, hd, what="") -> float:
    """got/before: [T, H*hd] bf16 after/before the rotation. The rotated dims
    are one bf16 rounding from the fp64 rotation; dims [rot:hd] keep their
    bits."""
    T = before.shape[0]
    rot = cos_sin.shape[1]
    ref, slack = ref_rope(positions, before, cos_sin, hd)
    g3 = got.detach().cpu().reshape(T, -1, hd)
    b3 = before.detach().cpu().reshape(T, -1, hd)
    assert_bits_equal(g3[..., rot:], b3[..., rot:], what + " dims [rot:hd]")
    return assert_bf16_rounded(got.detach().cpu().reshape(T, -1), ref, slack, what)


def ref_argmax(logits) -> torch.Tensor:
    """Smallest index of the row maximum (no NaNs), int64 [R]."""
    v = _cpu64(logits)
    m = v.amax(dim=1, keepdim=True)
    idx = torch.arange(v.shape[1]).expand_as(v)
    big = torch.full_like(idx, v.shape[1])
    return torch.where(v == m, idx, big).amin(dim=1)


def check_argmax(got, logits, what="") -> None:
    want = ref_argmax(logits)
    g = got.detach().cpu()
    assert g.dtype == torch.int64 and g.shape == want.shape, (g.dtype, g.shape)
    assert torch.equal(g, want), f"{what}: got {g.tolist()} want {want.tolist()}"


def greedy_rows(V: int, R: int, seed: int) -> torch.Tensor:
    """[R, V] bf16 logits (R = 1 or 5) with ties of the row maximum planted
    at indices that different lanes and different waves of the 256-thread
    block own, both when a thread reads 8 consecutive logits per pass and
    when it reads every 256th; the smallest tied index must win.
      row 0: ties at 25, 563, V//2 and V-1 (those below V)
      row 1: -inf except one entry near the end
      row 2: all -inf            -> 0
      row 3: constant            -> 0
      row 4: ties at V//2 and V-1 only, and a -inf head
    """
    assert R in (1, 5)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g).to(BF16)  # |x| < 7 < the planted 9
    for i in (25, 563, V // 2, V - 1):
        x[0, min(i, V - 1)] = 9.0
    if R == 5:
        x[1] = float("-inf")
        x[1, (3 * V) // 4] = -5.0
        x[2] = float("-inf")
        x[3] = 0.375
        x[4, : V // 4] = float("-inf")
        x[4, V // 2] = 9.0
        x[4, V - 1] = 9.0
    return x


def kv_rows(rows: int, hd: int, seed: int) -> torch.Tensor:
    """[rows, hd] bf16 for kv_quant. From 7 rows up: row 1 is all zero, row 2
    one-hot, and row 3 has amax = 127/32 and every other value an odd
    multiple of 1/64, so its scale is exactly 2^-5 and every quotient but the
    first is an exact tie (see assert_int8_codes)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, hd, generator=g) * 2).to(BF16)
    if rows >= 7:
        x[1] = 0
        x[2] = 0
        x[2, hd // 2] = -3.0
        k = torch.arange(hd) % 120 + 0.5
        k = torch.where(torch.arange(hd) % 2 == 0, k, -k)
        k[0] = 127.0
        x[3] = (k / 32).to(BF16)
    return x


def ref_lora_bgmv(out, x, A, B, scale, idx, col_off) -> torch.Tensor:
    """fp64 out with out[t, col_off:+W] += scale[s] * B[s] @ (A[s] @ x[t])
    for s = idx[t] >= 0."""
    o = _cpu64(out).clone()
    x64, A64, B64, sc = _cpu64(x), _cpu64(A), _cpu64(B), _cpu64(scale)
    W = B.shape[1]
    for t in range(x.shape[0]):
        s = int(idx[t])
        if s < 0:
            continue
        o[t, col_off : col_off + W] += sc[s] * (B64[s] @ (A64[s] @ x64[t]))
    return o


def lora_bgmv_fp32_kernel_order(out, x, A, B, scale, idx, col_off):
    """The same expression in fp32 in the order csrc/lora_bgmv.hip sums it,
    before the final rounding to bf16: lane l of a wave adds the products of
    elements l*8 + k*512 + j (k outer, j inner), the 64 lane sums meet in an
    XOR tree (offsets 32..1), y = sum * scale, then each column adds
    B[c, r] * y[r] for r = 0..R-1 and the old out value is added last.
    Returns fp32 [T, out_width]."""
    f32 = torch.float32
    o = out.detach().cpu().to(f32).clone()
    IN = x.shape[1]
    R = A.shape[1]
    W = B.shape[1]
    pad = (-IN) % 512
    lanes = torch.arange(64)
    for t in range(x.shape[0]):
        s = int(idx[t])
        if s < 0:
            continue
        a = torch.nn.functional.pad(A[s].detach().cpu().to(f32), (0, pad))
        xv = torch.nn.functional.pad(x[t].detach().cpu().to(f32), (0, pad))
        a = a.reshape(R, -1, 64, 8)  # [R, k, lane, j]
        xv = xv.reshape(-1, 64, 8)
        acc = torch.zeros(R, 64, dtype=f32)
        for k in range(a.shape[1]):
            for j in range(8):
                acc = acc + a[:, k, :, j] * xv[k, :, j]
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
        y = acc[:, 0] * scale.detach().cpu().to(f32)[s]
        b = B[s].detach().cpu().to(f32)  # [W, R]
        acc2 = torch.zeros(W, dtype=f32)
        for r in range(R):
            acc2 = acc2 + b[:, r] * y[r]
        o[t, col_off : col_off + W] = o[t, col_off : col_off + W] + acc2
    return o


def lora_measured_deviation(out, x, A, B, scale, idx, col_off) -> float:
    """Largest |fp32 kernel-order value - fp64 value| over out."""
    got = lora_bgmv_fp32_kernel_order(out, x, A, B, scale, idx, col_off)
    ref = ref_lora_bgmv(out, x, A, B, scale, idx, col_off)
    return float((got.to(F64) - ref).abs().max())


def check_lora_bgmv(got, out_before, x, A, B, scale, idx, col_off, slack,
                    what="") -> float:
    """The touched block is one bf16 rounding (+ slack) from the fp64 value;
    skipped rows and the columns outside [col_off, col_off + W) keep their
    bits."""
    W = B.shape[1]
    g = got.detach().cpu()
    before = out_before.detach().cpu()
    ref = ref_lora_bgmv(before, x, A, B, scale, idx, col_off)
    touched = torch.zeros(before.shape, dtype=torch.bool)
    rows = torch.as_tensor([int(i) >= 0 for i in idx], dtype=torch.bool)
    touched[rows, col_off : col_off + W] = True
    assert_bits_equal(
        torch.where(touched, torch.zeros_like(g), g),
        torch.where(touched, torch.zeros_like(before), before),
        what + " untouched elements",
    )
    if not touched.any():
        return 0.0
    return assert_bf16_rounded(g[touched], ref[touched], slack, what)


# ---------------------------------------------------------------------------
# lora_bgmv cases. `slack` is MEASURED, not derived: 4x the largest deviation
# of lora_bgmv_fp32_kernel_order from ref_lora_bgmv on exactly these inputs
# (lora_inputs with the case's seed). The CPU test recomputes it.
# ---------------------------------------------------------------------------
def lora_inputs(seed, T, IN, W, R, S, col_off, idx, x_pad=24, out_pad=40):
    """CPU tensors: x a strided row view of a wider buffer, out wider than
    col_off + W, A/B scaled so that the delta is O(0.3) like a served
    adapter's."""
    g = torch.Generator().manual_seed(seed)
    xbuf = torch.randn(T, IN + x_pad, generator=g).to(BF16)
    out = torch.randn(T, col_off + W + out_pad, generator=g).to(BF16)
    A = (torch.randn(S, R, IN, generator=g) * 0.05).to(BF16)
    B = (torch.randn(S, W, R, generator=g) * 0.05).to(BF16)
    scale = torch.rand(S, generator=g) + 0.5
    return dict(xbuf=xbuf, IN=IN, out=out, A=A, B=B, scale=scale,
                idx=torch.tensor(idx, dtype=torch.int32), col_off=col_off)


LORA_CASES = {
    # name: (kwargs for lora_inputs, slack)
    "in1024_w768_r16": (
        dict(seed=101, T=5, IN=1024, W=768, R=16, S=3, col_off=16,
             idx=[2, -1, 0, 1, 2]),
        1.05e-6,  # 4 x 2.61e-7 measured
    ),
    "in520_w100_r1": (  # IN off a multiple of 512, one rank row, W < block
        dict(seed=102, T=4, IN=520, W=100, R=1, S=2, col_off=0,
             idx=[-1, 1, 0, 1]),
        4.7e-7,  # 4 x 1.17e-7 measured
    ),
    "in4096_w1000_r6": (  # R off a multiple of the 4 waves, W off 256
        dict(seed=103, T=5, IN=4096, W=1000, R=6, S=3, col_off=16,
             idx=[0, 2, -1, 1, 0]),
        1.05e-6,  # 4 x 2.62e-7 measured
    ),
    "in1024_w256_r64": (  # largest supported rank
        dict(seed=104, T=3, IN=1024, W=256, R=64, S=2, col_off=0,
             idx=[1, -1, 0]),
        3.4e-6,  # 4 x 8.35e-7 measured
    ),
    "all_rows_skipped": (  # nothing is touched, so nothing to allow for
        dict(seed=105, T=4, IN=520, W=100, R=1, S=2, col_off=16,
             idx=[-1, -1, -1, -1]),
        0.0,
    ),
    # the shape of tests/test_kernels_gpu.py's original LoRA test
    "t33_in1024_w768_r16": (
        dict(seed=1, T=33, IN=1024, W=768, R=16, S=4, col_off=16,
             idx=[(7 * i) % 5 - 1 for i in range(33)], x_pad=0, out_pad=16),
        1.17e-6,  # 4 x 2.92e-7 measured
    ),
}


def lora_case(name):
    """(inputs dict on the CPU, slack) of a LORA_CASES entry; inputs["x"] is
    the strided view the kernel is given."""
    kw, slack = LORA_CASES[name]
    d = lora_inputs(**kw)
    d["x"] = d["xbuf"][:, : d["IN"]]
    return d, slack
