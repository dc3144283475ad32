"""gemm_w4_tiled (csrc/gemm_w4_tiled.hip) vs the fp64 reference and bound of
tests/test_gemm_w4_gpu.py: want = x.double() @ Wd.double().T on the
torch-built bf16 Wd, |got - want| <= 2^-8 |want| + K * 2^-24 * A, which holds
for any fp32 summation order and so covers split-K."""

import pytest
import torch

from production_stack_amd import ops
from tests.test_gemm_w4_gpu import G, _assert_within, _inputs, _operands, _wd

pytestmark = pytest.mark.gpu

SPLIT = (129, 128, 4096)
SHAPES = [
    (1, 64, 128),      # one row, a half N tile alone, one group: no loop
    (127, 128, 256), (128, 128, 256), (129, 128, 256),  # M tile edge
    (257, 192, 384),   # first M int4_linear sends here, N tail, 3 groups
    (300, 320, 512),   # 3 x 3 tiles with both tails
    SPLIT,             # split-K
    (129, 128, 128),   # units == 1: one split
]


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _splits(M, N, K):
    from production_stack_amd import _C

    return _C.gemm_w4_tiled_splits(M, N, K)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_numeric(M, N, K):
    if (M, N, K) == SPLIT:
        assert _splits(M, N, K) > 1
    if K == G:
        assert _splits(M, N, K) == 1
    x, packed, s, z = _inputs(M, N, K)
    _assert_within(ops.gemm_w4_tiled(x, packed, s, z), x, packed, s, z)


def test_exact():
    """test_gemm_w4_gpu.test_exact's construction at (300, 192, 384): every
    output is a sum of 16 terms d * s, a multiple of 0.5 of magnitude <= 64,
    exact in fp32 and bf16 in any order, so the result equals the fp64
    reference bit for bit. A wrong tile index, swizzle, nibble order or a
    swapped s/z fails."""
    M, N, K = 300, 192, 384
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
    want = x.double() @ _wd(q, s, z).double().T
    assert float(want.abs().max()) <= 64
    assert torch.equal(want, want.bfloat16().double()), "premise: exact"
    assert bool(want.any())
    got = ops.gemm_w4_tiled(x, ops.int4_pack(q), s, z)
    assert torch.equal(got.double(), want), (
        f"{int((got.double() != want).sum())}/{want.numel()} outputs differ "
        "from the exact result"
    )


def test_split_k_deterministic():
    x, packed, s, z = _inputs(*SPLIT)
    runs = [ops.gemm_w4_tiled(x, packed, s, z) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int16), runs[0].view(torch.int16))


def test_accept_rule():
    dims = (32, 64, 96, 128, 192, 256, 320, 384, 512, 4096, 14336)
    for M in (0, 1, 256, 257, 4096):
        for N in dims:
            for K in dims:
                assert ops.gemm_w4_tiled_supported(M, N, K) == (
                    _splits(M, N, K) > 0), (M, N, K)


def test_rejects_and_empty():
    for M, N, K in [(300, 96, 128), (300, 64, 192)]:
        with pytest.raises(RuntimeError):
            ops.gemm_w4_tiled(*_operands(M, N, K))
    with pytest.raises(RuntimeError):
        ops.gemm_w4_tiled(*_operands(300, 64, 256, x_dtype=torch.float16))
    out = ops.gemm_w4_tiled(*_operands(0, 64, 128))
    assert out.shape == (0, 64) and out.dtype == torch.bfloat16


def test_int4_linear_tiled_dispatch(monkeypatch):
    calls = {"int4_dequant": [], "skinny_gemm_w4": [], "gemm_w4_tiled": []}
    real = {name: getattr(ops, name) for name in calls}
    for name in calls:
        def shim(*a, _name=name):
            calls[_name].append(a[0].shape[0])
            return real[_name](*a)

        monkeypatch.setattr(ops, name, shim)

    x, packed, s, z = _inputs(300, 512, 1024)
    got = ops.int4_linear(x, packed, s, z, backend="tiled")
    assert calls == {"int4_dequant": [], "skinny_gemm_w4": [],
                     "gemm_w4_tiled": [300]}
    _assert_within(got, x, packed, s, z)

    x, packed, s, z = _inputs(96, 512, 1024)
    got = ops.int4_linear(x, packed, s, z, backend="tiled")
    assert calls["skinny_gemm_w4"] == [96] and calls["int4_dequant"] == []
    assert len(calls["gemm_w4_tiled"]) == 1
    want = real["skinny_gemm_w4"](x, packed, s, z)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))

    with pytest.raises(ValueError):
        ops.int4_linear(x, packed, s, z, backend="bogus")
