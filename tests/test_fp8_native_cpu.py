"""The fp8_gemm="native" setting without a GPU: config and CLI plumbing, the
accept rule's Python restatement, the CPU oracles, and a CPU engine that
holds per-channel scales."""

import inspect

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.sampling import SamplingParams
from production_stack_amd.ops import reference
from tests import elementwise_criteria as ec

FP8 = torch.float8_e4m3fn


def _engine(**kw):
    cfg = EngineConfig(
        model="tiny-llama",
        max_model_len=256,
        seed=3,
        cache=CacheConfig(num_gpu_blocks=64, block_size=16),
        scheduler=SchedulerConfig(max_num_seqs=4, max_num_batched_tokens=128),
        **kw,
    )
    return LLMEngine(cfg, device="cpu")


def test_default_is_scaled_mm():
    assert EngineConfig().fp8_gemm == "scaled_mm"
    sig = inspect.signature(ops.fp8_linear_rowwise)
    assert sig.parameters["backend"].default == "scaled_mm"


@pytest.mark.parametrize("quantization", [None, "fp8"])
def test_unknown_fp8_gemm_rejected(quantization):
    with pytest.raises(ValueError):
        _engine(quantization=quantization, fp8_gemm="cutlass")


def test_unknown_backend_argument_rejected():
    z = torch.zeros((1, 64), dtype=torch.float32).to(FP8)
    with pytest.raises(ValueError):
        ops.fp8_linear_rowwise(z, torch.ones(1), z, torch.ones(1),
                               backend="cutlass")


def test_server_cli_fp8_gemm():
    from production_stack_amd.engine.server import build_arg_parser

    ap = build_arg_parser()
    assert ap.parse_args([]).fp8_gemm == "scaled_mm"
    assert ap.parse_args(["--fp8-gemm", "scaled_mm"]).fp8_gemm == "scaled_mm"
    args = ap.parse_args(
        ["--quantization", "fp8", "--fp8-gemm", "native"])
    assert args.fp8_gemm == "native" and args.quantization == "fp8"
    with pytest.raises(SystemExit):
        ap.parse_args(["--fp8-gemm", "triton"])


@pytest.mark.parametrize(
    "M,N,K,want",
    [
        (0, 64, 64, False), (1, 64, 64, True), (256, 64, 64, True),
        (257, 64, 64, False),
        (16, 96, 64, False), (16, 128, 64, True), (16, 0, 64, False),
        (16, 64, 96, False), (16, 64, 128, True), (16, 64, 0, False),
    ],
)
def test_supported_truth_table(M, N, K, want):
    assert ops.skinny_gemm_fp8_supported(M, N, K) is want


def _quantized(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) / 8).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / 8).to(torch.bfloat16)
    xq, sx = reference.quant_fp8_rows(x)
    wq, sw = ops.fp8_quantize_weight_rowwise(w)
    return xq, sx, wq, sw


def test_reference_fp8_linear_rowwise():
    """fp32 dequant matmul vs fp64: one bf16 rounding (2^-9 relative) plus
    the fp32 dequantisation and K-term summation error, K * 2^-24 of the
    absolute-value product, as in tests/test_gemm_fp8_gpu.py."""
    M, N, K = 9, 64, 192
    xq, sx, wq, sw = _quantized(M, N, K, 11)
    got = reference.fp8_linear_rowwise(xq, sx, wq, sw)
    assert got.dtype == torch.bfloat16 and got.shape == (M, N)
    s = sx.double()[:, None] * sw.double()[None, :]
    want = (xq.double() @ wq.double().T) * s
    A = (xq.double().abs() @ wq.double().abs().T) * s
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -24 * A
    assert bool(((got.double() - want).abs() <= bound).all())
    # asymmetric scales: a transposed scale index would show
    assert not torch.equal(
        got, reference.fp8_linear_rowwise(xq, sx.flip(0), wq, sw))


def test_reference_quant_fp8_rows():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(7, 96, generator=g) * 3).to(torch.bfloat16)
    x[2] = 0
    before = x.clone()
    xq, sx = reference.quant_fp8_rows(x)
    assert xq.dtype == FP8 and sx.dtype == torch.float32
    ec.assert_fp8_rounded(xq, sx, x.double(), "reference.quant_fp8_rows")
    assert torch.equal(x, before)
    # ops dispatches CPU tensors to the reference
    xq2, sx2 = ops.quant_fp8_rows(x)
    ec.assert_bits_equal(xq2, xq)
    assert torch.equal(sx2, sx)


def test_cpu_engine_native_holds_channel_scales():
    eng = _engine(quantization="fp8", fp8_gemm="native")
    for layer in eng.runner.model.layers:
        assert layer.fp8_gemm == "native"
        for wq, sc in layer.fp8_w.values():
            assert wq.dtype == FP8
            assert sc.shape == (wq.shape[0],)
    p = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    out = eng.generate([list(range(20, 50))], p)["offline-0"]
    assert len(out) == 4
    # the default keeps per-tensor scales on the CPU
    base = _engine(quantization="fp8")
    for layer in base.runner.model.layers:
        assert all(sc.dim() == 0 for _, sc in layer.fp8_w.values())
