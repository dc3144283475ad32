"""skinny_gemm_fp8 and quant_fp8_rows vs fp64 references.

Reference for every tolerance case, as a GPU fp64 matmul (no in-tree kernel
involved):
    want = (xq.double() @ wq.double().T) * sx[:, None] * sw[None, :]

Tolerance, derived and not measured. With
    A = (|xq|.double() @ |wq|.double().T) * sx[:, None] * sw[None, :]
the bound is |got - want| <= 2^-8 * |want| + K * 2^-24 * A, elementwise.
The first term is twice the bf16 round-to-nearest bound (the scale product
and the scaling add two fp32 roundings, far below the other half). The second
is the standard fp32 recursive-summation bound over K products, which are
exact in fp32 for e4m3 operands; the split-K adds are covered by it. A
dropped or doubled 64-wide K-chunk moves an output by about sqrt(64) typical
products, far outside this. What a tolerance could still absorb is caught by
the exact-integer case, which asserts bit equality.

Inputs: x = randn/8 and w = randn/8 in bf16, seeded per shape; w quantized
with ops.fp8_quantize_weight_rowwise, x with ops.quant_fp8_rows.
"""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine.config import ARCHITECTURES
from tests import elementwise_criteria as ec

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn

MTILE = [(M, 128, 192) for M in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)]
POISON = [(16, 3072, 4096), (1, 6144, 768), (33, 2048, 5632)]
EXACT = (129, 128, 192)
SWEEP_M = (1, 16, 64, 256)


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _C():
    from production_stack_amd import _C as ext

    return ext


def _splits(M, N, K):
    return _C().skinny_gemm_fp8_splits(M, N, K)


def _inputs(M, N, K):
    torch.manual_seed(M * 1000003 + N * 1009 + K)
    x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 8
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
    wq, sw = ops.fp8_quantize_weight_rowwise(w)
    xq, sx = ops.quant_fp8_rows(x)
    return xq, sx, wq, sw


def _ref(xq, sx, wq, sw):
    s = sx.double()[:, None] * sw.double()[None, :]
    want = (xq.double() @ wq.double().T) * s
    A = (xq.double().abs() @ wq.double().abs().T) * s
    return want, A


def _assert_within(got, xq, sx, wq, sw):
    K = xq.shape[1]
    want, A = _ref(xq, sx, wq, sw)
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
    xq, sx, wq, sw = _inputs(M, N, K)
    _assert_within(ops.skinny_gemm_fp8(xq, sx, wq, sw), xq, sx, wq, sw)


# ----------------------------------------------------- split-K poison ----

def _poisoned_call(xq, sx, wq, sw):
    """Run the op with its split-K workspace landing on an all-NaN block."""
    M, K = xq.shape
    N = wq.shape[0]
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
    got = ops.skinny_gemm_fp8(xq, sx, wq, sw)
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
    xq, sx, wq, sw = _inputs(M, N, K)
    runs = [_poisoned_call(xq, sx, wq, sw) for _ in range(3)]
    _assert_within(runs[0], xq, sx, wq, sw)
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int16), runs[0].view(torch.int16)), (
            "repeated runs are not bit-identical"
        )


# ------------------------------------------------------ exact integers ----

def test_exact_integer():
    """64 ones per xq row and integer wq in [-2, 2], all exact in e4m3, with
    power-of-two scales that differ along rows (period 3) and columns
    (period 5): every output is an integer of magnitude <= 128 times a power
    of two, exact in fp32 and bf16 in any summation order, so the result
    must equal the fp64 reference bit for bit. A swapped or transposed scale
    index or a row<->col swap in the C write fails."""
    M, N, K = EXACT
    g = torch.Generator(device="cuda").manual_seed(M * 1000003 + N * 1009 + K)
    cols = torch.rand(M, K, device="cuda", generator=g).argsort(1)[:, :64]
    x = torch.zeros(M, K, device="cuda")
    x.scatter_(1, cols, 1.0)
    assert bool((x.sum(1) == 64).all())
    w = torch.randint(-2, 3, (N, K), device="cuda", generator=g).float()
    xq, wq = x.to(FP8), w.to(FP8)
    assert torch.equal(xq.float(), x) and torch.equal(wq.float(), w)
    sx = 2.0 ** ((torch.arange(M, device="cuda") % 3) - 1).float()
    sw = 2.0 ** ((torch.arange(N, device="cuda") % 5) - 2).float()
    want, _ = _ref(xq, sx, wq, sw)
    assert float((x.double() @ w.double().T).abs().max()) <= 128
    got = ops.skinny_gemm_fp8(xq, sx, wq, sw)
    assert torch.equal(got.double(), want), (
        f"{int((got.double() != want).sum())}/{want.numel()} outputs differ "
        "from the exact result"
    )


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
    per = ceil(units/splits), units = K // 64, so the last split is
    non-empty iff per*(splits-1) < units. An empty split returns before
    writing its workspace slice, which the combine kernel still sums. Also
    pins that the split count does not depend on M."""
    cases = {(M, N, K) for M in SWEEP_M for (N, K) in _preset_shapes()}
    cases |= set(MTILE + POISON + [EXACT])
    checked, bad = 0, []
    for (M, N, K) in sorted(cases):
        s = _splits(M, N, K)
        if s <= 0:
            continue
        checked += 1
        assert s == _splits(1, N, K), (M, N, K)
        units = K // 64
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
                assert ops.skinny_gemm_fp8_supported(M, N, K) == (
                    _splits(M, N, K) > 0), (M, N, K)


def _operands(M, N, K, x_dtype=FP8, n_sx=None):
    xq = torch.zeros((M, K), device="cuda").to(x_dtype)
    wq = torch.zeros((N, K), device="cuda").to(FP8)
    sx = torch.ones(M if n_sx is None else n_sx, device="cuda")
    sw = torch.ones(N, device="cuda")
    return xq, sx, wq, sw


@pytest.mark.parametrize("M,N,K", [(257, 64, 64), (16, 96, 64), (16, 64, 96)])
def test_rejects_shapes(M, N, K):
    with pytest.raises(RuntimeError):
        ops.skinny_gemm_fp8(*_operands(M, N, K))


def test_rejects_operands():
    with pytest.raises(RuntimeError):
        ops.skinny_gemm_fp8(*_operands(16, 64, 64, x_dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        ops.skinny_gemm_fp8(*_operands(16, 64, 64, n_sx=15))
    # the same operands, well-formed, are accepted
    out = ops.skinny_gemm_fp8(*_operands(16, 64, 64))
    assert out.shape == (16, 64) and not bool(out.any())


def test_empty_batch():
    out = ops.skinny_gemm_fp8(*_operands(0, 64, 64))
    assert out.shape == (0, 64) and out.dtype == torch.bfloat16


# ------------------------------------------------------ row independence ----

def test_row_independent_of_m():
    """Rows [:5] at M=40 (the 4-m-tile instantiation) equal the M=5 result
    (the 1-m-tile one) bit for bit: split depth depends on (N, K) only and
    every m-tile count accumulates in the same order."""
    N, K = 256, 4096
    xq, sx, wq, sw = _inputs(40, N, K)
    big = ops.skinny_gemm_fp8(xq, sx, wq, sw)
    small = ops.skinny_gemm_fp8(xq[:5].contiguous(), sx[:5].contiguous(),
                                wq, sw)
    ec.assert_bits_equal(big[:5], small, "rows [:5] of M=40 vs M=5")


# -------------------------------------------------------- quant_fp8_rows ----

def test_quant_fp8_rows():
    torch.manual_seed(37)
    x = torch.randn(37, 4096, dtype=torch.bfloat16, device="cuda") * 3
    x[5] = 0
    before = x.clone()
    xq, sx = ops.quant_fp8_rows(x)
    assert xq.dtype == FP8 and sx.dtype == torch.float32
    worst = ec.assert_fp8_rounded(xq, sx, x.double(), "quant_fp8_rows")
    print(f"quant_fp8_rows (37, 4096): worst {worst:.4f} half-steps")
    ec.assert_bits_equal(x, before, "quant_fp8_rows input")


def test_quant_fp8_rows_strided():
    torch.manual_seed(29)
    buf = torch.randn(29, 1536, dtype=torch.bfloat16, device="cuda")
    buf[3] = 0
    before = buf.clone()
    x = buf[:, 256:1280]
    assert x.shape == (29, 1024) and x.stride(0) == 1536
    xq, sx = ops.quant_fp8_rows(x)
    assert xq.is_contiguous()
    ec.assert_fp8_rounded(xq, sx, x.double(), "quant_fp8_rows strided")
    ec.assert_bits_equal(buf, before, "quant_fp8_rows strided input")


def test_quant_fp8_rows_rejects():
    x = torch.zeros((4, 12), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.quant_fp8_rows(x)


# ------------------------------------------------------ backend dispatch ----

def test_backend_dispatch(monkeypatch):
    calls = []
    real = ops.skinny_gemm_fp8

    def shim(*a):
        calls.append(a[0].shape[0])
        return real(*a)

    monkeypatch.setattr(ops, "skinny_gemm_fp8", shim)

    xq, sx, wq, sw = _inputs(96, 512, 1024)
    native = ops.fp8_linear_rowwise(xq, sx, wq, sw, backend="native")
    assert calls == [96]
    ec.assert_bits_equal(native, real(xq, sx, wq, sw), "native backend")
    _assert_within(native, xq, sx, wq, sw)

    del calls[:]
    default = ops.fp8_linear_rowwise(xq, sx, wq, sw)
    assert calls == [], "the default backend ran the native kernel"
    assert default.shape == native.shape

    # M above the kernel's range falls through to the default path
    xq, sx, wq, sw = _inputs(300, 512, 1024)
    big = ops.fp8_linear_rowwise(xq, sx, wq, sw, backend="native")
    assert calls == []
    ec.assert_bits_equal(big, ops.fp8_linear_rowwise(xq, sx, wq, sw),
                         "M=300 fallthrough")
