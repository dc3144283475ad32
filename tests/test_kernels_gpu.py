"""Numerics tests: every HIP kernel vs the plain-PyTorch fp32 reference.

All tests are gpu-marked; the references themselves are covered by CPU tests
elsewhere. Tolerances account for bf16 storage (~2^-8 relative).
"""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.ops import reference
from tests import elementwise_criteria as ec

pytestmark = pytest.mark.gpu


def setup_module(module):
    torch.manual_seed(0)
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("shape", [(7, 4096), (33, 8192), (1, 1024), (256, 4096)])
def test_rms_norm(shape):
    x = torch.randn(shape, dtype=torch.bfloat16, device="cuda")
    w = torch.randn(shape[-1], dtype=torch.bfloat16, device="cuda")
    got = ops.rms_norm(x, w, 1e-5)
    want = reference.rms_norm(x.cpu(), w.cpu(), 1e-5)
    _close(got, want)


@pytest.mark.parametrize("shape", [(13, 4096), (256, 8192)])
def test_fused_add_rms_norm(shape):
    x = torch.randn(shape, dtype=torch.bfloat16, device="cuda")
    res = torch.randn(shape, dtype=torch.bfloat16, device="cuda")
    w = torch.randn(shape[-1], dtype=torch.bfloat16, device="cuda")
    want_n, want_r = reference.fused_add_rms_norm(x.cpu(), res.cpu(), w.cpu(), 1e-5)
    got_n, got_r = ops.fused_add_rms_norm(x, res, w, 1e-5)
    _close(got_r, want_r)
    _close(got_n, want_n)


@pytest.mark.parametrize("shape", [(9, 11008), (128, 28672)])
def test_silu_and_mul(shape):
    t, d2 = shape
    x = torch.randn((t, d2 * 2), dtype=torch.bfloat16, device="cuda")
    got = ops.silu_and_mul(x)
    want = reference.silu_and_mul(x.cpu())
    _close(got, want)


@pytest.mark.parametrize("qh,kh,hd,rot", [(32, 8, 128, 128), (8, 1, 64, 64)])
def test_rope(qh, kh, hd, rot):
    T = 17
    max_pos = 512
    inv = 1.0 / (500000.0 ** (torch.arange(0, rot, 2).float() / rot))
    t = torch.arange(max_pos).float()
    freqs = torch.outer(t, inv)
    cos_sin = torch.cat([freqs.cos(), freqs.sin()], dim=-1).contiguous().cuda()
    pos = torch.randint(0, max_pos, (T,), dtype=torch.int32, device="cuda")
    q = torch.randn((T, qh * hd), dtype=torch.bfloat16, device="cuda")
    k = torch.randn((T, kh * hd), dtype=torch.bfloat16, device="cuda")
    want_q, want_k = reference.rotary_embedding(
        pos.cpu(), q.cpu(), k.cpu(), cos_sin.cpu(), hd
    )
    got_q, got_k = ops.rotary_embedding(pos, q, k, cos_sin, hd)
    _close(got_q, want_q)
    _close(got_k, want_k)


def _make_cache(nb, kh, bs, hd, device="cuda"):
    k_cache = torch.randn((nb, kh, bs, hd), dtype=torch.bfloat16, device=device)
    v_cache = torch.randn((nb, kh, bs, hd), dtype=torch.bfloat16, device=device)
    return k_cache, v_cache


def test_reshape_and_cache():
    nb, kh, bs, hd = 32, 8, 16, 128
    T = 40
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    kc_ref, vc_ref = k_cache.cpu().clone(), v_cache.cpu().clone()
    k = torch.randn((T, kh, hd), dtype=torch.bfloat16, device="cuda")
    v = torch.randn((T, kh, hd), dtype=torch.bfloat16, device="cuda")
    slots = torch.randperm(nb * bs)[:T].to(torch.long)
    slots[5] = -1  # skipped token
    reference.reshape_and_cache(k.cpu(), v.cpu(), kc_ref, vc_ref, slots)
    ops.reshape_and_cache(k, v, k_cache, v_cache, slots.cuda())
    _close(k_cache, kc_ref, atol=0, rtol=0)
    _close(v_cache, vc_ref, atol=0, rtol=0)


@pytest.mark.parametrize("qh,kh,hd", [(32, 8, 128), (8, 8, 128),
                                      (16, 2, 128), (8, 2, 64),
                                      (24, 8, 128), (28, 4, 128),
                                      (16, 8, 64)])
def test_paged_attn_decode(qh, kh, hd):
    torch.manual_seed(1)
    S, bs = 5, 16
    seq_lens = torch.tensor([1, 17, 33, 256, 100], dtype=torch.int32)
    max_blocks = 32
    nb = S * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
        S, max_blocks
    )
    q = torch.randn((S, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_decode(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), block_tables, seq_lens,
        1.0 / hd ** 0.5,
    )
    got = ops.paged_attn_decode(
        q, k_cache, v_cache, block_tables.cuda(), seq_lens.cuda(),
        1.0 / hd ** 0.5,
    )
    _close(got, want)


@pytest.mark.parametrize("num_splits", [1, 2, 4, 8, 32])
def test_paged_attn_decode_split_kv(num_splits):
    """All split factors must agree with the reference (incl. splits that
    exceed the block count of short sequences)."""
    from production_stack_amd import _C

    torch.manual_seed(3)
    qh, kh, hd, bs = 32, 8, 128, 16
    S = 4
    seq_lens = torch.tensor([5, 700, 64, 333], dtype=torch.int32)
    max_blocks = 44
    nb = S * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
        S, max_blocks
    )
    q = torch.randn((S, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_decode(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), block_tables, seq_lens,
        1.0 / hd ** 0.5,
    )
    out = torch.empty_like(q)
    _C.paged_attn_decode(
        out, q, k_cache, v_cache, block_tables.cuda(), seq_lens.cuda(),
        1.0 / hd ** 0.5, num_splits,
    )
    _close(out, want)


@pytest.mark.parametrize("qh,kh,hd", [(32, 8, 128), (4, 4, 64)])
def test_paged_attn_prefill(qh, kh, hd):
    torch.manual_seed(2)
    bs = 16
    # two sequences: one fresh prefill (pos 0..30), one chunked continuation
    # (pos 64..95 with 64 tokens of prior context in cache)
    seqs = [31, 32]
    start = [0, 64]
    max_blocks = 16
    nb = 2 * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, 2 * max_blocks + 1, dtype=torch.int32).reshape(
        2, max_blocks
    )
    token_seq = torch.cat(
        [torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(seqs)]
    )
    token_pos = torch.cat(
        [torch.arange(s, s + n, dtype=torch.int32) for s, n in zip(start, seqs)]
    )
    T = token_seq.shape[0]
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_prefill(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), block_tables, token_seq,
        token_pos, 1.0 / hd ** 0.5,
    )
    got = ops.paged_attn_prefill(
        q, k_cache, v_cache, block_tables.cuda(), token_seq.cuda(),
        token_pos.cuda(), 1.0 / hd ** 0.5,
    )
    _close(got, want)


def test_greedy_sample():
    R, V = 9, 128256
    logits = torch.randn((R, V), dtype=torch.bfloat16, device="cuda")
    got = ops.greedy_sample(logits)
    want = reference.greedy_sample(logits.cpu())
    assert torch.equal(got.cpu(), want)


def _build_tiles(chunks, tile=64):
    """chunks: list of (seq_row, start_pos, n_tokens) -> tiles + token maps"""
    tiles, token_seq, token_pos = [], [], []
    flat = 0
    for row, (r, start, n) in enumerate(chunks):
        for t0 in range(0, n, tile):
            tiles.append([r, flat + t0, start + t0, min(tile, n - t0)])
        for p in range(start, start + n):
            token_seq.append(r)
            token_pos.append(p)
        flat += n
    return (
        torch.tensor(tiles, dtype=torch.int32),
        torch.tensor(token_seq, dtype=torch.int32),
        torch.tensor(token_pos, dtype=torch.int32),
    )


@pytest.mark.parametrize("qh,kh", [(32, 8), (8, 8), (16, 2)])
def test_paged_attn_prefill_mfma(qh, kh):
    """MFMA prefill vs fp32 reference: fresh prefills, chunked continuations,
    ragged tile tails, multiple sequences."""
    torch.manual_seed(4)
    hd, bs = 128, 16
    # (seq_row, start_pos, n_tokens)
    chunks = [(0, 0, 200), (1, 128, 100), (2, 0, 1), (3, 31, 64)]
    max_blocks = 32
    nb = 4 * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, 4 * max_blocks + 1, dtype=torch.int32).reshape(
        4, max_blocks
    )
    tiles, token_seq, token_pos = _build_tiles(chunks)
    T = token_seq.shape[0]
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_prefill(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), block_tables, token_seq,
        token_pos, 1.0 / hd ** 0.5,
    )
    got = ops.paged_attn_prefill_mfma(
        q, k_cache, v_cache, block_tables.cuda(), tiles.cuda(),
        1.0 / hd ** 0.5,
    )
    _close(got, want)


def test_prefill_mfma_matches_valu_kernel():
    """Cross-check the two GPU prefill kernels against each other on a
    longer context."""
    torch.manual_seed(5)
    qh, kh, hd, bs = 32, 8, 128, 16
    chunks = [(0, 1024, 512)]
    max_blocks = 96
    nb = max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, max_blocks + 1, dtype=torch.int32).reshape(
        1, max_blocks
    )
    tiles, token_seq, token_pos = _build_tiles(chunks)
    T = token_seq.shape[0]
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    a = ops.paged_attn_prefill_mfma(
        q, k_cache, v_cache, block_tables.cuda(), tiles.cuda(), 0.0883883,
    )
    b = ops.paged_attn_prefill(
        q, k_cache, v_cache, block_tables.cuda(), token_seq.cuda(),
        token_pos.cuda(), 0.0883883,
    )
    _close(a, b, atol=3e-2, rtol=3e-2)


def test_fused_rope_cache_matches_separate_ops():
    from production_stack_amd import _C

    torch.manual_seed(6)
    T, qh, kh, hd, bs, nb = 23, 32, 8, 128, 16, 8
    rot = hd
    width = (qh + 2 * kh) * hd
    qkv = torch.randn((T, width), dtype=torch.bfloat16, device="cuda")
    inv = 1.0 / (500000.0 ** (torch.arange(0, rot, 2).float() / rot))
    freqs = torch.outer(torch.arange(4096).float(), inv)
    cos_sin = torch.cat([freqs.cos(), freqs.sin()], -1).contiguous().cuda()
    pos = torch.randint(0, 4096, (T,), dtype=torch.int32, device="cuda")
    slots = torch.randperm(nb * bs)[:T].to(torch.long).cuda()
    slots[3] = -1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    kc2, vc2 = k_cache.clone(), v_cache.clone()

    # reference composition: split -> rope -> reshape_and_cache
    qs, kvs = qh * hd, kh * hd
    q = qkv[:, :qs].contiguous()
    k = qkv[:, qs : qs + kvs].contiguous()
    v = qkv[:, qs + kvs :].contiguous()
    q_ref, k_ref = reference.rotary_embedding(
        pos.cpu(), q.cpu(), k.cpu(), cos_sin.cpu(), hd
    )
    kc2, vc2 = kc2.cpu(), vc2.cpu()
    reference.reshape_and_cache(
        k_ref.view(T, kh, hd), v.cpu().view(T, kh, hd), kc2, vc2, slots.cpu()
    )

    qkv_fused = qkv.clone()
    _C.fused_rope_cache(
        qkv_fused, pos, cos_sin, slots, k_cache, v_cache, qh, hd
    )
    _close(qkv_fused[:, :qs], q_ref)
    _close(qkv_fused[:, qs : qs + kvs], k_ref)
    _close(k_cache, kc2, atol=2e-2, rtol=2e-2)
    _close(v_cache, vc2, atol=0, rtol=0)


def test_paged_attn_decode_lowreg_variant():
    from production_stack_amd import _C

    torch.manual_seed(7)
    qh, kh, hd, bs = 32, 8, 128, 16
    S = 3
    seq_lens = torch.tensor([5, 700, 64], dtype=torch.int32)
    max_blocks = 44
    nb = S * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
        S, max_blocks
    )
    q = torch.randn((S, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_decode(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), block_tables, seq_lens,
        1.0 / hd ** 0.5,
    )
    out = torch.empty_like(q)
    _C.paged_attn_decode(
        out, q, k_cache, v_cache, block_tables.cuda(), seq_lens.cuda(),
        1.0 / hd ** 0.5, 0, 1,
    )
    _close(out, want)


def test_kv_quant_gpu_matches_reference():
    x = torch.randn(200, 128, dtype=torch.bfloat16, device="cuda") * 2
    q_gpu, s_gpu = ops.kv_quant(x)
    q_ref, s_ref = reference.kv_quant(x.cpu())
    torch.testing.assert_close(
        s_gpu.cpu(), s_ref, atol=1e-5, rtol=1e-4
    )
    # codes are round-half-even of the fp64 quotient; only near-ties may
    # differ by 1
    ec.assert_int8_codes(q_gpu, s_gpu, x, "kv_quant")
    diff = (q_gpu.cpu().int() - q_ref.int()).abs()
    assert diff.max() <= 1
    y = ops.kv_dequant(q_gpu, s_gpu)
    ec.assert_bits_equal(
        y, (q_gpu.cpu().float() * s_gpu.cpu()[:, None]).to(torch.bfloat16),
        "kv_dequant",
    )
    torch.testing.assert_close(
        y.float().cpu(), x.float().cpu(), atol=0.05, rtol=0.05
    )


@pytest.mark.parametrize("M,N,K", [
    (1, 6144, 4096), (16, 6144, 4096), (17, 4096, 4096),
    (64, 4096, 14336), (128, 28672, 4096), (100, 4096, 4096),
    (192, 6144, 4096), (256, 4096, 4096), (256, 28672, 4096),
    (250, 4096, 14336),
])
def test_skinny_gemm(M, N, K):
    torch.manual_seed(M)
    x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 8
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
    got = ops.skinny_gemm(x, w)
    want = (x.float() @ w.float().t()).to(torch.bfloat16)
    _close(got, want, atol=3e-2, rtol=3e-2)


def test_skinny_gemm_strided_x():
    """x as a strided row view (the qkv input is a slice of a wider buf)."""
    M, K, N = 32, 4096, 4096
    buf = torch.randn(M, K + 512, dtype=torch.bfloat16, device="cuda") / 8
    x = buf[:, :K]
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
    got = ops.skinny_gemm(x, w)
    want = (x.float() @ w.float().t()).to(torch.bfloat16)
    _close(got, want, atol=3e-2, rtol=3e-2)


def test_paged_attn_decode_fp8_kv():
    from production_stack_amd import _C

    torch.manual_seed(9)
    qh, kh, hd, bs = 32, 8, 128, 16
    S = 3
    seq_lens = torch.tensor([5, 300, 64], dtype=torch.int32)
    max_blocks = 20
    nb = S * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    k8 = k_cache.to(torch.float8_e4m3fn)
    v8 = v_cache.to(torch.float8_e4m3fn)
    block_tables = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
        S, max_blocks
    )
    q = torch.randn((S, qh, hd), dtype=torch.bfloat16, device="cuda")
    # reference on the DEQUANTIZED cache (fp8 is lossy by design)
    want = reference.paged_attn_decode(
        q.cpu(), k8.cpu().to(torch.bfloat16), v8.cpu().to(torch.bfloat16),
        block_tables, seq_lens, 1.0 / hd ** 0.5,
    )
    out = torch.empty_like(q)
    _C.paged_attn_decode(
        out, q, k8, v8, block_tables.cuda(), seq_lens.cuda(),
        1.0 / hd ** 0.5, 0, 1,
    )
    _close(out, want, atol=3e-2, rtol=3e-2)


def test_paged_attn_prefill_mfma_fp8_kv():
    from production_stack_amd import _C

    torch.manual_seed(10)
    qh, kh, hd, bs = 32, 8, 128, 16
    chunks = [(0, 0, 150), (1, 64, 80)]
    max_blocks = 16
    nb = 2 * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    k8 = k_cache.to(torch.float8_e4m3fn)
    v8 = v_cache.to(torch.float8_e4m3fn)
    block_tables = torch.arange(1, 2 * max_blocks + 1, dtype=torch.int32).reshape(
        2, max_blocks
    )
    tiles, token_seq, token_pos = _build_tiles(chunks)
    T = token_seq.shape[0]
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_prefill(
        q.cpu(), k8.cpu().to(torch.bfloat16), v8.cpu().to(torch.bfloat16),
        block_tables, token_seq, token_pos, 1.0 / hd ** 0.5,
    )
    out = torch.empty_like(q)
    _C.paged_attn_prefill_mfma(
        out, q, k8, v8, block_tables.cuda(), tiles.cuda(),
        1.0 / hd ** 0.5, 3,
    )
    _close(out, want, atol=3e-2, rtol=3e-2)


def test_fused_rope_cache_fp8():
    from production_stack_amd import _C

    torch.manual_seed(11)
    T, qh, kh, hd, bs, nb = 9, 8, 4, 128, 16, 4
    width = (qh + 2 * kh) * hd
    qkv = torch.randn((T, width), dtype=torch.bfloat16, device="cuda")
    inv = 1.0 / (500000.0 ** (torch.arange(0, hd, 2).float() / hd))
    freqs = torch.outer(torch.arange(64).float(), inv)
    cos_sin = torch.cat([freqs.cos(), freqs.sin()], -1).contiguous().cuda()
    pos = torch.randint(0, 64, (T,), dtype=torch.int32, device="cuda")
    slots = torch.randperm(nb * bs)[:T].to(torch.long).cuda()
    k8 = torch.zeros(nb, kh, bs, hd, dtype=torch.float8_e4m3fn, device="cuda")
    v8 = torch.zeros_like(k8)
    kb = torch.zeros(nb, kh, bs, hd, dtype=torch.bfloat16, device="cuda")
    vb = torch.zeros_like(kb)
    qkv2 = qkv.clone()
    _C.fused_rope_cache(qkv2, pos, cos_sin, slots, kb, vb, qh, hd)
    _C.fused_rope_cache(qkv.clone(), pos, cos_sin, slots, k8, v8, qh, hd)
    _close(k8.to(torch.bfloat16), kb, atol=4e-2, rtol=6e-2)
    _close(v8.to(torch.bfloat16), vb, atol=4e-2, rtol=6e-2)


def test_engine_fp8_kv_e2e():
    from production_stack_amd.engine.config import (
        CacheConfig,
        EngineConfig,
        SchedulerConfig,
    )
    from production_stack_amd.engine.engine import LLMEngine
    from production_stack_amd.engine.sampling import SamplingParams

    def run(kv_dtype):
        cfg = EngineConfig(
            model="mini-llama",
            max_model_len=1024,
            seed=7,
            cache=CacheConfig(num_gpu_blocks=128, block_size=16,
                              kv_cache_dtype=kv_dtype),
            scheduler=SchedulerConfig(max_num_seqs=8,
                                      max_num_batched_tokens=1024),
        )
        eng = LLMEngine(cfg, device="cuda")
        assert eng.runner.graphs is not None, (
            f"hipGraph capture must succeed with kv dtype {kv_dtype}"
        )
        p = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
        return eng.generate([list(range(40, 140))], p)["offline-0"]

    bf = run("auto")
    f8 = run("fp8_e4m3")
    assert len(f8) == 12
    # random-init logits are argmax-noise-sensitive; fp8 KV is lossy by
    # design, so only require early-token agreement
    agree = sum(a == b for a, b in zip(bf[:4], f8[:4]))
    assert agree >= 2, (bf, f8)


def test_lora_bgmv_kernel_matches_reference():
    """T=33, IN=1024, W=768, R=16 at col_off 16: the touched block within one
    bf16 rounding (plus the measured fp32 slack of this case) of the fp64
    value, everything else untouched."""
    d, slack = ec.lora_case("t33_in1024_w768_r16")
    out = d["out"].cuda()
    ops.lora_bgmv(out, d["x"].cuda(), d["A"].cuda(), d["B"].cuda(),
                  d["scale"].cuda(), d["idx"].cuda(), col_off=d["col_off"])
    torch.cuda.synchronize()
    ec.check_lora_bgmv(out, d["out"], d["x"], d["A"], d["B"], d["scale"],
                       d["idx"], d["col_off"], slack, "lora_bgmv")
    want = d["out"].clone()
    reference.lora_bgmv(want, d["x"], d["A"], d["B"], d["scale"], d["idx"],
                        d["col_off"])
    diff = (out.cpu().float() - want.float()).abs().max()
    assert diff < 0.25, f"max diff {diff}"


def test_windowed_decode_matches_reference():
    from production_stack_amd.ops import reference

    torch.manual_seed(21)
    qh, kh, hd, bs = 8, 2, 128, 16
    S, max_blocks, W = 3, 24, 80
    seq_lens = torch.tensor([30, 300, 150], dtype=torch.int32)
    nb = S * max_blocks + 1
    k_cache = torch.randn(nb, kh, bs, hd, dtype=torch.bfloat16,
                          device="cuda") / 4
    v_cache = torch.randn_like(k_cache) / 4
    bt = torch.arange(1, S * max_blocks + 1, dtype=torch.int32,
                      device="cuda").view(S, max_blocks)
    q = torch.randn(S, qh, hd, dtype=torch.bfloat16, device="cuda") / 4
    got = ops.paged_attn_decode(q, k_cache, v_cache, bt,
                                seq_lens.cuda(), 0.0883, window=W)
    want = reference.paged_attn_decode(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), bt.cpu(), seq_lens,
        0.0883, window=W)
    _close(got.cpu(), want, atol=2e-2, rtol=2e-2)


def test_windowed_prefill_mfma_matches_reference():
    from production_stack_amd.ops import reference

    torch.manual_seed(22)
    qh, kh, hd, bs = 8, 2, 128, 16
    W = 64
    ctx = 256
    nb = ctx // bs + 1
    k_cache = torch.randn(nb, kh, bs, hd, dtype=torch.bfloat16,
                          device="cuda") / 4
    v_cache = torch.randn_like(k_cache) / 4
    bt = torch.arange(1, nb, dtype=torch.int32, device="cuda").view(1, -1)
    q = torch.randn(ctx, qh, hd, dtype=torch.bfloat16, device="cuda") / 4
    tiles = []
    for t0 in range(0, ctx, 64):
        tiles.append([0, t0, t0, min(64, ctx - t0)])
    tile_info = torch.tensor(tiles, dtype=torch.int32, device="cuda")
    got = ops.paged_attn_prefill_mfma(q, k_cache, v_cache, bt, tile_info,
                                      0.0883, window=W)
    token_seq = torch.zeros(ctx, dtype=torch.int32)
    token_pos = torch.arange(ctx, dtype=torch.int32)
    want = reference.paged_attn_prefill(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), bt.cpu(), token_seq,
        token_pos, 0.0883, window=W)
    _close(got.cpu(), want, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("qh,kh", [(32, 8), (16, 2)])
def test_prefill_mfma32_v5_vs_reference(qh, kh):
    """v5 (8-wave 32x32 swapped-QK^T, 256-row tiles) vs fp32 reference:
    fresh prefill, chunked continuation, ragged tails, 1-token chunk."""
    torch.manual_seed(40)
    hd, bs = 128, 16
    chunks = [(0, 0, 600), (1, 256, 300), (2, 0, 1), (3, 100, 130)]
    max_blocks = 64
    nb = 4 * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    block_tables = torch.arange(1, 4 * max_blocks + 1, dtype=torch.int32).reshape(
        4, max_blocks
    )
    tiles, token_seq, token_pos = _build_tiles(
        chunks, tile=ops.prefill_tile_rows(qh, kh))
    T = token_seq.shape[0]
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_prefill(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), block_tables, token_seq,
        token_pos, 1.0 / hd ** 0.5,
    )
    got = ops.paged_attn_prefill_mfma(
        q, k_cache, v_cache, block_tables.cuda(), tiles.cuda(),
        1.0 / hd ** 0.5, variant=5,
    )
    _close(got, want)


def test_prefill_mfma32_v5_matches_v3():
    torch.manual_seed(41)
    qh, kh, hd = 32, 8, 128
    chunks = [(0, 2048, 1024)]
    max_blocks = 192
    nb = max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, 16, hd)
    block_tables = torch.arange(1, max_blocks + 1, dtype=torch.int32).reshape(
        1, max_blocks
    )
    t5, _, _ = _build_tiles(chunks, tile=ops.prefill_tile_rows(qh, kh))
    t3, _, _ = _build_tiles(chunks, tile=64)
    T = 1024
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    a = ops.paged_attn_prefill_mfma(
        q, k_cache, v_cache, block_tables.cuda(), t5.cuda(), 0.0883883,
        variant=5,
    )
    b = ops.paged_attn_prefill_mfma(
        q, k_cache, v_cache, block_tables.cuda(), t3.cuda(), 0.0883883,
        variant=3,
    )
    _close(a, b, atol=3e-2, rtol=3e-2)


def test_prefill_mfma32_v5_fp8_kv():
    from production_stack_amd import _C

    torch.manual_seed(42)
    qh, kh, hd, bs = 32, 8, 128, 16
    chunks = [(0, 0, 300), (1, 64, 80)]
    max_blocks = 32
    nb = 2 * max_blocks + 1
    k_cache, v_cache = _make_cache(nb, kh, bs, hd)
    k8 = k_cache.to(torch.float8_e4m3fn)
    v8 = v_cache.to(torch.float8_e4m3fn)
    block_tables = torch.arange(1, 2 * max_blocks + 1, dtype=torch.int32).reshape(
        2, max_blocks
    )
    tiles, token_seq, token_pos = _build_tiles(
        chunks, tile=ops.prefill_tile_rows(qh, kh))
    T = token_seq.shape[0]
    q = torch.randn((T, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_prefill(
        q.cpu(), k8.cpu().to(torch.bfloat16), v8.cpu().to(torch.bfloat16),
        block_tables, token_seq, token_pos, 1.0 / hd ** 0.5,
    )
    out = torch.empty_like(q)
    _C.paged_attn_prefill_mfma(
        out, q, k8, v8, block_tables.cuda(), tiles.cuda(),
        1.0 / hd ** 0.5, 5,
    )
    _close(out, want, atol=3e-2, rtol=3e-2)


def test_prefill_mfma32_v5_windowed():
    from production_stack_amd.ops import reference

    torch.manual_seed(43)
    qh, kh, hd, bs = 8, 2, 128, 16
    W = 160
    ctx = 640
    nb = ctx // bs + 1
    k_cache = torch.randn(nb, kh, bs, hd, dtype=torch.bfloat16,
                          device="cuda") / 4
    v_cache = torch.randn_like(k_cache) / 4
    bt = torch.arange(1, nb, dtype=torch.int32, device="cuda").view(1, -1)
    q = torch.randn(ctx, qh, hd, dtype=torch.bfloat16, device="cuda") / 4
    tr = ops.prefill_tile_rows(qh, kh)
    tiles = []
    for t0 in range(0, ctx, tr):
        tiles.append([0, t0, t0, min(tr, ctx - t0)])
    tile_info = torch.tensor(tiles, dtype=torch.int32, device="cuda")
    got = ops.paged_attn_prefill_mfma(q, k_cache, v_cache, bt, tile_info,
                                      0.0883, window=W, variant=5)
    token_seq = torch.zeros(ctx, dtype=torch.int32)
    token_pos = torch.arange(ctx, dtype=torch.int32)
    want = reference.paged_attn_prefill(
        q.cpu(), k_cache.cpu(), v_cache.cpu(), bt.cpu(), token_seq,
        token_pos, 0.0883, window=W)
    _close(got.cpu(), want, atol=3e-2, rtol=3e-2)


def test_rms_norm_fp8_fused_act_quant():
    """Fused (add-)RMSNorm -> fp8 + row scales: every code within one e4m3
    rounding of the fp64 norm over the emitted scale, the scale amax/448,
    and in the fused form the residual updated and x left alone."""
    torch.manual_seed(50)
    for fused in (False, True):
        T, D = 37, 4096
        x = torch.randn(T, D, dtype=torch.bfloat16, device="cuda")
        res = torch.randn(T, D, dtype=torch.bfloat16, device="cuda")
        w = torch.randn(D, dtype=torch.bfloat16, device="cuda")
        if fused:
            x2, r2 = x.clone(), res.clone()
            want, r_want = ops.fused_add_rms_norm(x2, r2, w, 1e-5)
            x_in, r_io = x.clone(), res.clone()
            xq, sx = ops.rms_norm_fp8(x_in, w, 1e-5, residual=r_io)
            ec.assert_bits_equal(r_io, ec.residual_sum_bf16(x, res),
                                 "new residual")
            ec.assert_bits_equal(r_io, r_want, "residual vs bf16 kernel")
            ec.assert_bits_equal(x_in, x, "x must stay as it was")
            ref = ec.ref_rms_norm(x, w, 1e-5, residual=res)
        else:
            want = ops.rms_norm(x, w, 1e-5)
            xq, sx = ops.rms_norm_fp8(x, w, 1e-5)
            ref = ec.ref_rms_norm(x, w, 1e-5)
        ec.assert_fp8_rounded(xq, sx, ref, f"rms_norm_fp8 fused={fused}")
        got = xq.float() * sx[:, None]
        err = (got - want.float()).abs()
        # fp8 e4m3 has a 3-bit mantissa: ~6.25% relative resolution
        tol = 0.08 * want.float().abs() + sx[:, None] * 2
        assert int((err > tol).sum()) == 0, err.max()


def test_silu_and_mul_fp8():
    torch.manual_seed(51)
    T, D = 29, 14336
    x = torch.randn(T, 2 * D, dtype=torch.bfloat16, device="cuda")
    want = ops.silu_and_mul(x)
    aq, sa = ops.silu_and_mul_fp8(x)
    ec.assert_fp8_rounded(aq, sa, ec.ref_silu_and_mul(x), "silu_and_mul_fp8")
    got = aq.float() * sa[:, None]
    err = (got - want.float()).abs()
    tol = 0.08 * want.float().abs() + sa[:, None] * 2
    assert int((err > tol).sum()) == 0, err.max()


def test_fp8_linear_rowwise_matches_reference():
    torch.manual_seed(52)
    M, N, K = 96, 512, 1024
    x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 4
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 4
    w_q, sw = ops.fp8_quantize_weight_rowwise(w)
    sx = (x.abs().amax(dim=1).float().clamp(min=1e-6) / 448.0)
    xq = (x.float() / sx[:, None]).to(torch.float8_e4m3fn)
    got = ops.fp8_linear_rowwise(xq, sx, w_q, sw).float().cpu()
    want = (x.float() @ w.float().t()).cpu()
    _close(got, want, atol=0.4, rtol=0.1)
