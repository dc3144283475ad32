"""skinny_gemm_w4, int4_dequant and the int4 packer vs fp64 references.

Format: W_deq[n, k] = bf16_rne(float(q[n, k] - z[n, k/128]) * float(s[n,
k/128])) with q, z in 0..15 and s bf16. The fp32 product is exact (a 5-bit
integer times an 8-bit significand), so the bf16 round is the only one, and
the reference below builds the same bf16 matrix in torch with no in-tree
kernel:
    Wd   = ((q.float() - z_expanded.float()) * s_expanded.float()).bfloat16()
    want = x.double() @ Wd.double().T
    A    = |x|.double() @ |Wd|.double().T

Tolerance, derived and not measured (the derivation of test_gemm_fp8_gpu.py):
    |got - want| <= 2^-8 * |want| + K * 2^-24 * A, elementwise.
The kernel's operands are the bf16 values of x and Wd, and bf16 x bf16
products are exact in fp32. The second term is the standard fp32
recursive-summation bound over K exact products; the split-K adds are covered
by it. The first term is twice the bf16 round-to-nearest bound of the one
final rounding. A dropped or doubled 128-wide group, a wrong scale or zero
point moves an output far outside this; what a tolerance could still absorb
is caught by the exact case, which asserts bit equality.

Inputs: x = randn/8 and w = randn/8 in bf16, seeded per shape; w quantized
with ops.int4_quantize_weight.
"""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine.config import ARCHITECTURES
from tests import elementwise_criteria as ec

pytestmark = pytest.mark.gpu

G = 128  # the kernel's K unit: one quantization group per split unit

MTILE = [(M, 128, 256) for M in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)]
POISON = [(16, 3072, 4096), (1, 6144, 768), (33, 2048, 5632)]
EXACT = (129, 128, 384)
SWEEP_M = (1, 16, 64, 256)


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _C():
    from production_stack_amd import _C as ext

    return ext


def _splits(M, N, K):
    return _C().skinny_gemm_w4_splits(M, N, K)


def _inputs(M, N, K):
    torch.manual_seed(M * 1000003 + N * 1009 + K)
    x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 8
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
    packed, s, z = ops.int4_quantize_weight(w)
    assert packed.shape == (N, K // 2) and packed.dtype == torch.uint8
    assert s.shape == (N, K // G) and s.dtype == torch.bfloat16
    assert z.shape == (N, K // G) and z.dtype == torch.uint8
    return x, packed, s, z


def _wd(q, s, z):
    """The dequantized bf16 matrix, from logical q, in plain torch."""
    ze = z.float().repeat_interleave(G, dim=1)
    se = s.float().repeat_interleave(G, dim=1)
    return ((q.float() - ze) * se).bfloat16()


def _ref(x, packed, s, z):
    Wd = _wd(ops.int4_unpack(packed), s, z)
    want = x.double() @ Wd.double().T
    A = x.double().abs() @ Wd.double().abs().T
    return want, A


def _assert_within(got, x, packed, s, z):
    K = x.shape[1]
    want, A = _ref(x, packed, s, z)
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    assert bool(torch.isfinite(got).all()), (
        f"{int((~torch.isfinite(got)).sum())}/{got.numel()} outputs are "
        "not finite"
    )
    err = (got.double() - want).abs()
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -24 * A
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"worst error {worst:.3f} x bound at {tuple(got.shape)} K={K}")
    bad = err > bound
    assert not bool(bad.any()), (
        f"{int(bad.sum())}/{bad.numel()} outputs beyond the bound; worst "
        f"{worst:.3f}x"
    )


# ------------------------------------------------------------ m-tiles ----

@pytest.mark.parametrize("M,N,K", MTILE)
def test_m_tile_edges(M, N, K):
    x, packed, s, z = _inputs(M, N, K)
    _assert_within(ops.skinny_gemm_w4(x, packed, s, z), x, packed, s, z)


# ----------------------------------------------------- split-K poison ----

def _poisoned_call(x, packed, s, z):
    """Run the op with its split-K workspace landing on an all-NaN block."""
    M, K = x.shape
    N = packed.shape[0]
    splits = _splits(M, N, K)
    assert splits > 1, "case must take the split-K workspace path"
    n = splits * M * N
    # keeps a block of the output's size free so the op's `out` allocation
    # (made before the workspace) cannot take the poisoned block
    spacer = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    poison = torch.full((n,), float("nan"), dtype=torch.float32,
                        device="cuda")
    ptr = poison.data_ptr()
    del poison
    again = torch.empty(n, dtype=torch.float32, device="cuda")
    # premise: an uninitialised allocation of the workspace's size gets the
    # NaN block back
    assert again.data_ptr() == ptr, "allocator did not reuse the block"
    assert bool(torch.isnan(again).all()), "reused block is not all-NaN"
    del again
    del spacer
    got = ops.skinny_gemm_w4(x, packed, s, z)
    # the op's workspace is free again: the same request must lead back to
    # the poisoned block, now holding the first split's finite partials
    probe = torch.empty(n, dtype=torch.float32, device="cuda")
    assert probe.data_ptr() == ptr, "workspace did not use the NaN block"
    assert bool(torch.isfinite(probe[: M * N]).all()), (
        "split 0 of the workspace was not written"
    )
    del probe
    return got


@pytest.mark.parametrize("M,N,K", POISON)
def test_poisoned_workspace(M, N, K):
    x, packed, s, z = _inputs(M, N, K)
    runs = [_poisoned_call(x, packed, s, z) for _ in range(3)]
    _assert_within(runs[0], x, packed, s, z)
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int16), runs[0].view(torch.int16)), (
            "repeated runs are not bit-identical"
        )


# ---------------------------------------------------------- exact case ----

def test_exact():
    """16 ones per x row; q = z + d with d in [-2, 2], z = 7 + (n + g) % 3
    and s = 2^(((n + 2g) % 3) - 1) for row n and group g of three. Every
    output is a sum of 16 terms d * s, a multiple of 0.5 of magnitude <= 64:
    exact in fp32 and bf16 in any summation order, so the result must equal
    the fp64 reference bit for bit. A wrong group index, a swapped s/z, a
    nibble-order slip or a row<->col swap fails."""
    M, N, K = EXACT
    gen = torch.Generator(device="cuda").manual_seed(
        M * 1000003 + N * 1009 + K)
    cols = torch.rand(M, K, device="cuda", generator=gen).argsort(1)[:, :16]
    x = torch.zeros(M, K, device="cuda")
    x.scatter_(1, cols, 1.0)
    assert bool((x.sum(1) == 16).all())
    x = x.bfloat16()
    n = torch.arange(N, device="cuda")[:, None]
    g = torch.arange(K // G, device="cuda")[None, :]
    z = (7 + (n + g) % 3).to(torch.uint8)
    s = (2.0 ** (((n + 2 * g) % 3) - 1).float()).bfloat16()
    d = torch.randint(-2, 3, (N, K), device="cuda", generator=gen)
    q = (z.long().repeat_interleave(G, dim=1) + d).to(torch.uint8)
    assert int(q.min()) >= 0 and int(q.max()) <= 15
    packed = ops.int4_pack(q)
    Wd = _wd(q, s, z)
    want = x.double() @ Wd.double().T
    assert float(want.abs().max()) <= 64
    assert torch.equal(want, want.bfloat16().double()), "premise: exact"
    assert bool(want.any())
    got = ops.skinny_gemm_w4(x, packed, s, z)
    assert torch.equal(got.double(), want), (
        f"{int((got.double() != want).sum())}/{want.numel()} outputs differ "
        "from the exact result"
    )


# ------------------------------------------------------ row independence ----

def test_row_independent_of_m():
    """Rows [:5] at M=40 (the 4-m-tile instantiation) equal the M=5 result
    (the 1-m-tile one) bit for bit: split depth depends on (N, K) only and
    every m-tile count accumulates in the same order."""
    N, K = 256, 4096
    x, packed, s, z = _inputs(40, N, K)
    big = ops.skinny_gemm_w4(x, packed, s, z)
    small = ops.skinny_gemm_w4(x[:5].contiguous(), packed, s, z)
    ec.assert_bits_equal(big[:5], small, "rows [:5] of M=40 vs M=5")


# ------------------------------------------------------------- dequant ----

@pytest.mark.parametrize("N,K", [(64, 128), (40, 384), (1000, 256)])
def test_int4_dequant(N, K):
    """Bit-equal to the torch formula; N need not be a multiple of 64 (only
    the GEMM has the N rule), and more than one block of the grid."""
    _, packed, s, z = _inputs(1, 64 * ((N + 63) // 64), K)
    packed, s, z = (t[:N].contiguous() for t in (packed, s, z))
    Wd = _wd(ops.int4_unpack(packed), s, z)
    got = ops.int4_dequant(packed, s, z)
    assert got.shape == (N, K) and got.dtype == torch.bfloat16
    ec.assert_bits_equal(got, Wd, f"int4_dequant {(N, K)}")
    ec.assert_bits_equal(
        ops.int4_dequant(packed.cpu(), s.cpu(), z.cpu()), Wd.cpu(),
        "reference int4_dequant",
    )


# --------------------------------------------------------- pack / unpack ----

def test_pack_unpack():
    gen = torch.Generator().manual_seed(5)
    q = torch.randint(0, 16, (37, 384), dtype=torch.uint8, generator=gen)
    p_cpu = ops.int4_pack(q)
    p_gpu = ops.int4_pack(q.cuda())
    assert p_cpu.shape == (37, 192) and p_cpu.dtype == torch.uint8
    assert p_gpu.is_cuda and torch.equal(p_gpu.cpu(), p_cpu)
    assert torch.equal(ops.int4_unpack(p_cpu), q)
    assert torch.equal(ops.int4_unpack(p_gpu).cpu(), q)


# ------------------------------------------------------------ host only ----

def _preset_shapes():
    """(N, K) of every projection of every model preset at TP 1, 2, 4, 8,
    sharded as engine/models/llama.py shards them."""
    shapes = set()
    for cfg in ARCHITECTURES.values():
        for tp in (1, 2, 4, 8):
            if cfg.num_q_heads % tp or cfg.intermediate_size % tp:
                continue
            if cfg.num_kv_heads % tp and tp % cfg.num_kv_heads:
                continue
            h = cfg.hidden_size
            qs = cfg.num_q_heads // tp * cfg.head_dim
            kvs = max(cfg.num_kv_heads // tp, 1) * cfg.head_dim
            inter = cfg.intermediate_size // tp
            shapes |= {
                (qs + 2 * kvs, h), (h, qs), (2 * inter, h), (h, inter),
                (cfg.vocab_size, h),
            }
    return sorted(shapes)


def test_no_empty_split():
    """Split s covers units [s*per, min(units, (s+1)*per)) with
    per = ceil(units/splits), units = K // 128 (the kernel splits K in whole
    quantization groups), so the last split is non-empty iff
    per*(splits-1) < units. An empty split returns before writing its
    workspace slice, which the combine kernel still sums. Also pins that the
    split count does not depend on M."""
    cases = {(M, N, K) for M in SWEEP_M for (N, K) in _preset_shapes()}
    cases |= set(MTILE + POISON + [EXACT])
    checked, bad = 0, []
    for (M, N, K) in sorted(cases):
        s = _splits(M, N, K)
        if s <= 0:
            continue
        checked += 1
        assert s == _splits(1, N, K), (M, N, K)
        units = K // G
        per = -(-units // s)
        if not per * (s - 1) < units:
            bad.append((M, N, K, s, per, -(-units // per)))
    assert checked > 100
    assert not bad, (
        f"{len(bad)}/{checked} shapes launch empty splits; first "
        f"(M, N, K, splits, per_split, non-empty): {bad[:8]}"
    )


def test_accept_rule():
    dims = (32, 64, 96, 128, 192, 256, 320, 384, 512, 4096, 14336)
    for M in (0, 1, 16, 64, 256, 257, 512, 1024):
        for N in dims:
            for K in dims:
                assert ops.skinny_gemm_w4_supported(M, N, K) == (
                    _splits(M, N, K) > 0), (M, N, K)


def _operands(M, N, K, x_dtype=torch.bfloat16, groups=None):
    x = torch.zeros((M, K), device="cuda").to(x_dtype)
    packed = torch.zeros((N, K // 2), dtype=torch.uint8, device="cuda")
    ng = K // G if groups is None else groups
    s = torch.ones((N, ng), dtype=torch.bfloat16, device="cuda")
    z = torch.zeros((N, K // G), dtype=torch.uint8, device="cuda")
    return x, packed, s, z


@pytest.mark.parametrize("M,N,K",
                         [(257, 64, 128), (16, 96, 128), (16, 64, 192)])
def test_rejects_shapes(M, N, K):
    with pytest.raises(RuntimeError):
        ops.skinny_gemm_w4(*_operands(M, N, K))


def test_rejects_operands():
    with pytest.raises(RuntimeError):
        ops.skinny_gemm_w4(*_operands(16, 64, 256, x_dtype=torch.float16))
    with pytest.raises(RuntimeError):
        ops.skinny_gemm_w4(*_operands(16, 64, 256, groups=1))
    # the same operands, well-formed, are accepted
    out = ops.skinny_gemm_w4(*_operands(16, 64, 256))
    assert out.shape == (16, 64) and not bool(out.any())


def test_empty_batch():
    out = ops.skinny_gemm_w4(*_operands(0, 64, 128))
    assert out.shape == (0, 64) and out.dtype == torch.bfloat16


# ------------------------------------------------------------- dispatch ----

def test_int4_linear_dispatch(monkeypatch):
    """int4_linear runs the native kernel inside the accept rule and
    int4_dequant + the bf16 GEMM outside it (M > 256)."""
    native, deq = [], []
    real_gemm, real_deq = ops.skinny_gemm_w4, ops.int4_dequant

    def gemm_shim(*a):
        native.append(a[0].shape[0])
        return real_gemm(*a)

    def deq_shim(*a):
        deq.append(tuple(a[0].shape))
        return real_deq(*a)

    monkeypatch.setattr(ops, "skinny_gemm_w4", gemm_shim)
    monkeypatch.setattr(ops, "int4_dequant", deq_shim)

    x, packed, s, z = _inputs(96, 512, 1024)
    got = ops.int4_linear(x, packed, s, z)
    assert native == [96] and deq == []
    ec.assert_bits_equal(got, real_gemm(x, packed, s, z), "native path")

    del native[:]
    x, packed, s, z = _inputs(300, 512, 1024)
    big = ops.int4_linear(x, packed, s, z)
    assert native == [] and deq == [(512, 512)]
    _assert_within(big, x, packed, s, z)
