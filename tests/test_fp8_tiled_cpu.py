"""The fp8_gemm="native_tiled" setting without a GPU: config and CLI
plumbing, the accept rule's Python restatement, and a CPU engine that holds
per-channel scales."""

import pytest

from production_stack_amd import ops
from tests.test_fp8_native_cpu import FP8, _engine


def test_config_and_cli_accept_native_tiled():
    from production_stack_amd.engine.server import build_arg_parser

    ap = build_arg_parser()
    args = ap.parse_args(["--quantization", "fp8", "--fp8-gemm",
                          "native_tiled"])
    assert args.fp8_gemm == "native_tiled"
    assert ap.parse_args([]).fp8_gemm == "scaled_mm"
    assert ops.FP8_TILED_MIN_M == 257
    with pytest.raises(ValueError):
        _engine(quantization="fp8", fp8_gemm="native_tilde")


def test_cpu_engine_holds_channel_scales():
    eng = _engine(quantization="fp8", fp8_gemm="native_tiled")
    for layer in eng.runner.model.layers:
        assert layer.fp8_gemm == "native_tiled"
        for wq, sc in layer.fp8_w.values():
            assert wq.dtype == FP8
            assert sc.shape == (wq.shape[0],)


@pytest.mark.parametrize(
    "M,N,K,want",
    [
        (0, 64, 64, False), (1, 64, 64, True), (256, 64, 64, True),
        (257, 64, 64, True), (1 << 20, 64, 64, True),
        (300, 96, 64, False), (300, 128, 64, True), (300, 0, 64, False),
        (300, 64, 96, False), (300, 64, 128, True), (300, 64, 0, False),
    ],
)
def test_supported_truth_table(M, N, K, want):
    assert ops.gemm_fp8_tiled_supported(M, N, K) is want
