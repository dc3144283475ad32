"""gemm_fp8_tiled (csrc/gemm_fp8_tiled.hip) vs the fp64 reference and bound of
tests/test_gemm_fp8_gpu.py: |got - want| <= 2^-8 |want| + K * 2^-24 * A, which
holds for any fp32 summation order and so covers split-K and the 128-deep
MFMA."""

import pytest
import torch

from production_stack_amd import ops
from tests.test_gemm_fp8_gpu import (
    FP8, _assert_within, _inputs, _operands, _ref,
)

pytestmark = pytest.mark.gpu

SPLIT = (129, 128, 4096)
SHAPES = [
    (1, 64, 64),       # one row, a half N tile, a lone half k-step: no loop
    (127, 128, 192), (128, 128, 192), (129, 128, 192),  # M tile edge, K tail
    (257, 192, 320),   # first M the dispatcher sends here, N tail, K tail,
                       # double-buffer wrap
    (300, 320, 512),   # 3 x 3 tiles with both tails
    SPLIT,             # split-K
    (129, 128, 128),   # one k-step: one split
]


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _splits(M, N, K):
    from production_stack_amd import _C

    return _C.gemm_fp8_tiled_splits(M, N, K)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_numeric(M, N, K):
    if (M, N, K) == SPLIT:
        assert _splits(M, N, K) > 1
    if K == 128:
        assert _splits(M, N, K) == 1
    xq, sx, wq, sw = _inputs(M, N, K)
    _assert_within(ops.gemm_fp8_tiled(xq, sx, wq, sw), xq, sx, wq, sw)


def test_exact():
    """test_gemm_fp8_gpu.test_exact_integer's construction at (300, 192,
    320): every output is an integer of magnitude <= 128 times a power of
    two, exact in fp32 and bf16 in any order, so the result equals the fp64
    reference bit for bit. A wrong tile index, swizzle, tail fill or scale
    index fails."""
    M, N, K = 300, 192, 320
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
    assert bool(want.any())
    got = ops.gemm_fp8_tiled(xq, sx, wq, sw)
    assert torch.equal(got.double(), want), (
        f"{int((got.double() != want).sum())}/{want.numel()} outputs differ "
        "from the exact result"
    )


def test_split_k_deterministic():
    xq, sx, wq, sw = _inputs(*SPLIT)
    runs = [ops.gemm_fp8_tiled(xq, sx, wq, sw) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int16), runs[0].view(torch.int16))


def test_accept_rule():
    dims = (32, 64, 96, 128, 192, 256, 320, 384, 512, 4096, 14336)
    for M in (0, 1, 256, 257, 4096):
        for N in dims:
            for K in dims:
                assert ops.gemm_fp8_tiled_supported(M, N, K) == (
                    _splits(M, N, K) > 0), (M, N, K)
    # split s covers k-steps [s*per, min(units, (s+1)*per)): none is empty
    for (M, N, K) in SHAPES:
        s, units = _splits(M, N, K), -(-K // 128)
        per = -(-units // s)
        assert per * (s - 1) < units, (M, N, K, s)


def test_rejects_and_empty():
    for M, N, K in [(300, 96, 64), (300, 64, 96)]:
        with pytest.raises(RuntimeError):
            ops.gemm_fp8_tiled(*_operands(M, N, K))
    with pytest.raises(RuntimeError):
        ops.gemm_fp8_tiled(*_operands(300, 64, 64, x_dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        ops.gemm_fp8_tiled(*_operands(300, 64, 64, n_sx=299))
    out = ops.gemm_fp8_tiled(*_operands(0, 64, 64))
    assert out.shape == (0, 64) and out.dtype == torch.bfloat16


def test_native_tiled_dispatch(monkeypatch):
    calls = {"skinny_gemm_fp8": [], "gemm_fp8_tiled": []}
    real = {name: getattr(ops, name) for name in calls}
    for name in calls:
        def shim(*a, _name=name):
            calls[_name].append(a[0].shape[0])
            return real[_name](*a)

        monkeypatch.setattr(ops, name, shim)

    xq, sx, wq, sw = _inputs(300, 512, 1024)
    got = ops.fp8_linear_rowwise(xq, sx, wq, sw, backend="native_tiled")
    assert calls == {"skinny_gemm_fp8": [], "gemm_fp8_tiled": [300]}
    _assert_within(got, xq, sx, wq, sw)

    xq, sx, wq, sw = _inputs(96, 512, 1024)
    got = ops.fp8_linear_rowwise(xq, sx, wq, sw, backend="native_tiled")
    assert calls == {"skinny_gemm_fp8": [96], "gemm_fp8_tiled": [300]}
    want = ops.fp8_linear_rowwise(xq, sx, wq, sw, backend="native")
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
