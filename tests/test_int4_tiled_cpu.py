"""The int4_gemm="tiled" plumbing that needs no GPU."""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine.config import EngineConfig
from production_stack_amd.engine.server import build_arg_parser
from production_stack_amd.ops import reference


def test_int4_linear_backend_on_cpu():
    torch.manual_seed(3)
    x = torch.randn(300, 256, dtype=torch.bfloat16) / 8
    w4 = ops.int4_quantize_weight(torch.randn(64, 256).bfloat16() / 8)
    want = reference.int4_linear(x, *w4)
    for backend in ("dequant", "tiled"):
        assert torch.equal(ops.int4_linear(x, *w4, backend=backend), want)
    with pytest.raises(ValueError):
        ops.int4_linear(x, *w4, backend="bogus")
    assert ops.INT4_TILED_MIN_M == 257
    assert ops.gemm_w4_tiled_supported(300, 64, 256)
    assert not ops.gemm_w4_tiled_supported(300, 96, 256)


def test_config_default_and_cli_flag():
    assert EngineConfig(model="mini-llama").int4_gemm == "dequant"
    ap = build_arg_parser()
    assert ap.parse_args([]).int4_gemm == "dequant"
    assert ap.parse_args(["--int4-gemm", "tiled"]).int4_gemm == "tiled"
    with pytest.raises(SystemExit):
        ap.parse_args(["--int4-gemm", "bogus"])
