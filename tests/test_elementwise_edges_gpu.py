"""Norm, activation, RoPE, KV-append, quantization, LoRA and sampling kernels
at the edges of their dispatch, against the fp64 references and the
one-rounding criteria of tests/elementwise_criteria.py (which
tests/test_elementwise_criteria_cpu.py shows reject subtly wrong kernels).

Inputs are generated on the CPU from a per-test seed and copied over, so the
references see exactly the kernels' inputs. Each test prints its worst figure
in units of its bound before it returns.
"""

import pytest
import torch

from production_stack_amd import ops
from tests import elementwise_criteria as ec

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
EPS = 1e-5


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _C():
    from production_stack_amd import _C as ext

    return ext


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _norm_rows(T, D, seed):
    """x, residual, w on the CPU: row 1 all zero (in x and residual), row 2
    scaled by 3e4."""
    g = _gen(seed)
    x = torch.randn(T, D, generator=g).to(BF16)
    res = torch.randn(T, D, generator=g).to(BF16)
    w = torch.randn(D, generator=g).to(BF16)
    x[1] = 0
    res[1] = 0
    x[2] = (x[2].float() * 3e4).to(BF16)
    return x, res, w


# ---------------------------------------------------------------------------
# rms_norm / fused_add_rms_norm: D = 8 (one thread), both sides of the
# 4096|4104 and 8192|8200 dispatch edges, 5120 (threads with differing vector
# counts) and the 32768 capacity.
# ---------------------------------------------------------------------------
NORM_DIMS = [8, 1024, 4096, 4104, 5120, 8192, 8200, 32768]


@pytest.mark.parametrize("D", NORM_DIMS)
def test_rms_norm_edges(D):
    x, _, w = _norm_rows(5, D, seed=1000 + D)
    got = ops.rms_norm(x.cuda(), w.cuda(), EPS)
    worst = ec.assert_bf16_rounded(got, ec.ref_rms_norm(x, w, EPS), 0.0,
                                   f"rms_norm D={D}")
    print(f"rms_norm D={D}: worst {worst:.4f} of the bound")


@pytest.mark.parametrize("D", NORM_DIMS)
def test_fused_add_rms_norm_edges(D):
    x, res, w = _norm_rows(5, D, seed=2000 + D)
    xg, rg = x.cuda(), res.cuda()
    got_n, got_r = ops.fused_add_rms_norm(xg, rg, w.cuda(), EPS)
    ec.assert_bits_equal(got_r, ec.residual_sum_bf16(x, res), "new residual")
    worst = ec.assert_bf16_rounded(
        got_n, ec.ref_rms_norm(x, w, EPS, residual=res), 0.0,
        f"fused_add_rms_norm D={D}")
    print(f"fused_add_rms_norm D={D}: worst {worst:.4f} of the bound")


# ---------------------------------------------------------------------------
# silu_and_mul: (300, 14336) has T*D/8 = 537600 > 2048*256 vectors, so the
# grid-stride loop runs a second time.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,D", [(3, 8), (5, 11008), (300, 14336)])
def test_silu_and_mul_edges(T, D):
    g = _gen(3000 + D)
    x = torch.randn(T, 2 * D, generator=g).to(BF16)
    x[0, :4] = torch.tensor([30.0, -30.0, 80.0, -80.0]).to(BF16)
    x[T - 1, D - 4 : D] = torch.tensor([-80.0, 80.0, -30.0, 30.0]).to(BF16)
    got = ops.silu_and_mul(x.cuda())
    worst = ec.assert_bf16_rounded(got, ec.ref_silu_and_mul(x), 0.0,
                                   f"silu_and_mul {T}x{D}")
    print(f"silu_and_mul {T}x{D}: worst {worst:.4f} of the bound")


# ---------------------------------------------------------------------------
# RoPE: partial rotary, (QH+KH)*rot/2 below and above the 256-thread block
# ---------------------------------------------------------------------------
ROPE_DIMS = [(128, 128), (128, 64), (64, 32), (64, 64)]
ROPE_HEADS = [(2, 1), (32, 8)]  # (2+1)*rot/2 <= 192 < 256 <= (32+8)*rot/2
MAX_POS = 97


def _rope_inputs(T, width, seed):
    g = _gen(seed)
    x = torch.randn(T, width, generator=g).to(BF16)
    pos = torch.randint(0, MAX_POS, (T,), generator=g, dtype=torch.int32)
    pos[0] = 0
    pos[1] = MAX_POS - 1
    return x, pos


@pytest.mark.parametrize("qh,kh", ROPE_HEADS)
@pytest.mark.parametrize("hd,rot", ROPE_DIMS)
def test_rotary_embedding_edges(hd, rot, qh, kh):
    T = 5
    x, pos = _rope_inputs(T, (qh + kh) * hd, seed=4000 + hd + rot + qh)
    q, k = x[:, : qh * hd].contiguous(), x[:, qh * hd :].contiguous()
    cs = ec.rope_table(MAX_POS, rot)
    got_q, got_k = ops.rotary_embedding(pos.cuda(), q.cuda(), k.cuda(),
                                        cs.cuda(), hd)
    wq = ec.check_rope(got_q, q, pos, cs, hd, "q")
    wk = ec.check_rope(got_k, k, pos, cs, hd, "k")
    print(f"rope hd={hd} rot={rot} heads={qh}+{kh}: worst {max(wq, wk):.4f}")


def _random_cache(nb, kh, bs, hd, dtype, seed):
    c = torch.randn(nb, kh, bs, hd, generator=_gen(seed)).to(BF16)
    return c.to(dtype)


def _scatter(cache, rows, slots, bs):
    """cache[slot // bs, :, slot % bs, :] = rows[t] for slots[t] >= 0, on the
    CPU; rows [T, KH, HD] already in the cache's dtype."""
    assert rows.dtype == cache.dtype
    bits = torch.uint8 if cache.dtype == FP8 else torch.int16
    out = cache.clone().view(bits)
    keep = slots >= 0
    s = slots[keep]
    out[s // bs, :, s % bs, :] = rows.contiguous().view(bits)[keep]
    return out.view(cache.dtype)


@pytest.mark.parametrize("cache_dtype", [BF16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("qh,kh", ROPE_HEADS)
@pytest.mark.parametrize("hd,rot", ROPE_DIMS)
def test_fused_rope_cache_edges(hd, rot, qh, kh, cache_dtype):
    T, bs, nb = 5, 16, 3
    width = (qh + 2 * kh) * hd
    qkv, pos = _rope_inputs(T, width, seed=5000 + hd + rot + qh)
    cs = ec.rope_table(MAX_POS, rot)
    slots = torch.tensor([17, 3, -1, 47, 0], dtype=torch.long)
    kc = _random_cache(nb, kh, bs, hd, cache_dtype, 1)
    vc = _random_cache(nb, kh, bs, hd, cache_dtype, 2)
    qkv_g, kc_g, vc_g = qkv.cuda(), kc.cuda(), vc.cuda()
    ops.fused_rope_cache(qkv_g, pos.cuda(), cs.cuda(), slots.cuda(), kc_g,
                         vc_g, qh, hd)
    after = qkv_g.cpu()
    qk = (qh + kh) * hd
    worst = ec.check_rope(after[:, :qk].contiguous(), qkv[:, :qk].contiguous(),
                          pos, cs, hd, "q|k in qkv")
    ec.assert_bits_equal(after[:, qk:], qkv[:, qk:], "v in qkv")
    # the cache rows are the rotated k written back into qkv, and v, cast to
    # the cache's dtype; everything else (the -1 slot too) keeps its bits
    k_rows = after[:, qh * hd : qk].reshape(T, kh, hd).to(cache_dtype)
    v_rows = qkv[:, qk:].reshape(T, kh, hd).to(cache_dtype)
    ec.assert_bits_equal(kc_g, _scatter(kc, k_rows, slots, bs), "k_cache")
    ec.assert_bits_equal(vc_g, _scatter(vc, v_rows, slots, bs), "v_cache")
    print(f"fused_rope_cache hd={hd} rot={rot}: worst {worst:.4f}")


# ---------------------------------------------------------------------------
# reshape_and_cache: (2050, 16, 128) has T*KH*HD/8 = 524800 > 2048*256
# vectors, so the grid-stride loop runs a second time.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cache_dtype", [BF16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("T,kh,hd", [(7, 2, 64), (7, 2, 128), (2050, 16, 128)])
def test_reshape_and_cache_edges(T, kh, hd, cache_dtype):
    bs = 16
    nb = (T + bs - 1) // bs + 2
    g = _gen(6000 + T + hd)
    k = torch.randn(T, kh, hd, generator=g).to(BF16)
    v = torch.randn(T, kh, hd, generator=g).to(BF16)
    slots = torch.randperm(nb * bs, generator=g)[:T].to(torch.long)
    slots[T // 2] = -1
    slots[T - 1] = -1
    kc = _random_cache(nb, kh, bs, hd, cache_dtype, 3)
    vc = _random_cache(nb, kh, bs, hd, cache_dtype, 4)
    kc_g, vc_g = kc.cuda(), vc.cuda()
    ops.reshape_and_cache(k.cuda(), v.cuda(), kc_g, vc_g, slots.cuda())
    ec.assert_bits_equal(kc_g, _scatter(kc, k.to(cache_dtype), slots, bs),
                         "k_cache")
    ec.assert_bits_equal(vc_g, _scatter(vc, v.to(cache_dtype), slots, bs),
                         "v_cache")


# ---------------------------------------------------------------------------
# greedy_sample: V = 8 (less than one pass), V % 8 != 0 (1000 is a multiple
# of 8; 50257 is not: rows after the first start off a 16-byte boundary and
# take the per-element loop), ties, -inf rows.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("V", [8, 1000, 2056, 50257, 128256])
def test_greedy_sample_edges(V, R):
    x = ec.greedy_rows(V, R, seed=7000 + V + R)
    ec.check_argmax(ops.greedy_sample(x.cuda()), x, f"V={V} R={R}")


@pytest.mark.parametrize("V", [1001, 2051])
def test_greedy_sample_odd_vocab(V):
    """Odd V: every second row starts on an odd 2-byte offset."""
    x = ec.greedy_rows(V, 5, seed=7500 + V)
    ec.check_argmax(ops.greedy_sample(x.cuda()), x, f"V={V}")


# ---------------------------------------------------------------------------
# kv_quant / kv_dequant: hd below one pass of the 64 lanes, two passes
# (1024), rows off a multiple of the 4 rows per block.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 203])
@pytest.mark.parametrize("hd", [8, 64, 128, 1024])
def test_kv_quant_dequant_edges(hd, rows):
    x = ec.kv_rows(rows, hd, seed=8000 + hd + rows)
    q, s = ops.kv_quant(x.cuda())
    assert q.shape == x.shape and s.shape == (rows,)
    ties = ec.assert_int8_codes(q, s, x, f"kv_quant hd={hd} rows={rows}")
    print(f"kv_quant hd={hd} rows={rows}: {ties} near-tie codes off by one")
    y = ops.kv_dequant(q, s)
    want = (q.cpu().float() * s.cpu()[:, None]).to(BF16)
    ec.assert_bits_equal(y, want, "kv_dequant")


# ---------------------------------------------------------------------------
# rms_norm_fp8: D <= 4096 is the <512, 1> instantiation, above it <1024, 2>
# up to its capacity of 16384.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("D", [8, 4096, 4104, 5120, 8192, 16384])
def test_rms_norm_fp8_edges(D, fused):
    x, res, w = _norm_rows(4, D, seed=9000 + D)
    xg, rg = x.cuda(), res.cuda()
    if fused:
        codes, scales = ops.rms_norm_fp8(xg, w.cuda(), EPS, residual=rg)
        ec.assert_bits_equal(rg, ec.residual_sum_bf16(x, res), "new residual")
        ref = ec.ref_rms_norm(x, w, EPS, residual=res)
    else:
        codes, scales = ops.rms_norm_fp8(xg, w.cuda(), EPS)
        ref = ec.ref_rms_norm(x, w, EPS)
    ec.assert_bits_equal(xg, x, "x must stay as it was")
    worst = ec.assert_fp8_rounded(codes, scales, ref, f"rms_norm_fp8 D={D}")
    print(f"rms_norm_fp8 D={D} fused={fused}: worst {worst:.4f} half-steps")


@pytest.mark.parametrize("D", [8, 4096, 4104, 14336, 32768])
def test_silu_and_mul_fp8_edges(D):
    g = _gen(9500 + D)
    x = torch.randn(4, 2 * D, generator=g).to(BF16)
    x[0, :4] = torch.tensor([30.0, -30.0, 80.0, -80.0]).to(BF16)
    x[1, :D] = 0  # silu(0) * up = 0: an all-zero output row
    codes, scales = ops.silu_and_mul_fp8(x.cuda())
    worst = ec.assert_fp8_rounded(codes, scales, ec.ref_silu_and_mul(x),
                                  f"silu_and_mul_fp8 D={D}")
    print(f"silu_and_mul_fp8 D={D}: worst {worst:.4f} half-steps")


# ---------------------------------------------------------------------------
# lora_bgmv (cases and their measured slack: elementwise_criteria.LORA_CASES)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ec.LORA_CASES))
def test_lora_bgmv_edges(name):
    d, slack = ec.lora_case(name)
    out_g = d["out"].cuda()
    x_g = d["xbuf"].cuda()[:, : d["IN"]]  # strided row view
    assert not x_g.is_contiguous() or d["xbuf"].shape[1] == d["IN"]
    ops.lora_bgmv(out_g, x_g, d["A"].cuda(), d["B"].cuda(), d["scale"].cuda(),
                  d["idx"].cuda(), col_off=d["col_off"])
    worst = ec.check_lora_bgmv(out_g, d["out"], d["x"], d["A"], d["B"],
                               d["scale"], d["idx"], d["col_off"], slack, name)
    print(f"lora_bgmv {name}: worst {worst:.4f} of the bound")


# ---------------------------------------------------------------------------
# Argument checks: every call below must fail on the host, before a launch.
# ---------------------------------------------------------------------------
def _bf(*shape):
    return torch.zeros(*shape, dtype=BF16, device="cuda")


def _fp8_out(T, D):
    return (torch.empty(T, D, dtype=FP8, device="cuda"),
            torch.empty(T, dtype=torch.float32, device="cuda"))


def test_row_capacity_is_enforced():
    """One vector past the largest instantiation of each row-in-registers
    kernel."""
    C = _C()
    D = 32768 + 8
    with pytest.raises(RuntimeError):
        C.rms_norm(_bf(1, D), _bf(1, D), _bf(D), EPS)
    with pytest.raises(RuntimeError):
        C.fused_add_rms_norm(_bf(1, D), _bf(1, D), _bf(D), EPS)
    with pytest.raises(RuntimeError):
        C.silu_and_mul_fp8(*_fp8_out(1, D), _bf(1, 2 * D))
    D = 16384 + 8
    for fused in (0, 1):
        with pytest.raises(RuntimeError):
            C.rms_norm_fp8(*_fp8_out(1, D), _bf(1, D), _bf(1, D), _bf(D), EPS,
                           fused)
    torch.cuda.synchronize()


def test_vector_width_is_enforced():
    C = _C()
    D = 12
    with pytest.raises(RuntimeError):
        C.rms_norm(_bf(1, D), _bf(1, D), _bf(D), EPS)
    with pytest.raises(RuntimeError):
        C.fused_add_rms_norm(_bf(1, D), _bf(1, D), _bf(D), EPS)
    with pytest.raises(RuntimeError):
        C.rms_norm_fp8(*_fp8_out(1, D), _bf(1, D), _bf(1, D), _bf(D), EPS, 0)
    with pytest.raises(RuntimeError):
        C.silu_and_mul_fp8(*_fp8_out(1, D), _bf(1, 2 * D))
    with pytest.raises(RuntimeError):
        C.kv_dequant(_bf(4, D),
                     torch.zeros(4, D, dtype=torch.int8, device="cuda"),
                     torch.ones(4, device="cuda"))
    torch.cuda.synchronize()


def _lora_args(IN=1024, W=64, R=8, T=2, S=2, x_width=None):
    xbuf = _bf(T, x_width or IN)
    return dict(
        out=_bf(T, W), x=xbuf[:, :IN], A=_bf(S, R, IN), B=_bf(S, W, R),
        scale=torch.ones(S, device="cuda"),
        idx=torch.zeros(T, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("kw", [dict(IN=1020), dict(R=65),
                                dict(x_width=1028)],
                         ids=["IN=1020", "R=65", "x_stride=1028"])
def test_lora_bgmv_rejects(kw):
    a = _lora_args(**kw)
    with pytest.raises(RuntimeError):
        _C().lora_bgmv(a["out"], a["x"], a["A"], a["B"], a["scale"], a["idx"], 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rot", [63, 256], ids=["odd", "above_hd"])
def test_rotary_dim_is_checked(rot):
    C = _C()
    T, qh, kh, hd, bs = 2, 2, 1, 128, 16
    pos = torch.zeros(T, dtype=torch.int32, device="cuda")
    cs = torch.zeros(8, rot, device="cuda")
    with pytest.raises(RuntimeError):
        C.rotary_embedding(pos, _bf(T, qh * hd), _bf(T, kh * hd), cs, hd)
    slots = torch.zeros(T, dtype=torch.long, device="cuda")
    kc, vc = _bf(1, kh, bs, hd), _bf(1, kh, bs, hd)
    with pytest.raises(RuntimeError):
        C.fused_rope_cache(_bf(T, (qh + 2 * kh) * hd), pos, cs, slots, kc, vc,
                           qh, hd)
    torch.cuda.synchronize()


def test_weight_and_output_shapes_are_checked():
    C = _C()
    T, D = 2, 1024
    with pytest.raises(RuntimeError):  # w shorter than a row
        C.rms_norm(_bf(T, D), _bf(T, D), _bf(D - 8), EPS)
    with pytest.raises(RuntimeError):
        C.fused_add_rms_norm(_bf(T, D), _bf(T, D), _bf(D - 8), EPS)
    with pytest.raises(RuntimeError):
        C.fused_add_rms_norm(_bf(T, D), _bf(T - 1, D), _bf(D), EPS)
    with pytest.raises(RuntimeError):
        C.rms_norm(_bf(T - 1, D), _bf(T, D), _bf(D), EPS)
    q, s = _fp8_out(T, D)
    with pytest.raises(RuntimeError):
        C.rms_norm_fp8(q, s, _bf(T, D), _bf(T, D), _bf(D - 8), EPS, 0)
    with pytest.raises(RuntimeError):  # out_q narrower than x
        C.rms_norm_fp8(_fp8_out(T, D - 8)[0], s, _bf(T, D), _bf(T, D), _bf(D),
                       EPS, 0)
    with pytest.raises(RuntimeError):  # one scale short
        C.rms_norm_fp8(q, s[:1], _bf(T, D), _bf(T, D), _bf(D), EPS, 0)
    with pytest.raises(RuntimeError):  # residual of another shape
        C.rms_norm_fp8(q, s, _bf(T, D), _bf(T - 1, D), _bf(D), EPS, 1)
    with pytest.raises(RuntimeError):
        C.silu_and_mul_fp8(_fp8_out(T, D - 8)[0], s, _bf(T, 2 * D))
    with pytest.raises(RuntimeError):  # out_q of the wrong dtype
        C.silu_and_mul_fp8(_bf(T, D), s, _bf(T, 2 * D))
    with pytest.raises(RuntimeError):
        C.kv_quant(torch.zeros(T, D - 8, dtype=torch.int8, device="cuda"),
                   torch.ones(T, device="cuda"), _bf(T, D))
    torch.cuda.synchronize()
