"""int4 (W4A16) MoE experts on the CPU: ops and a mini-mixtral engine."""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine import config
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.sampling import SamplingParams
from production_stack_amd.ops import reference


def test_cpu_path_is_reference_on_dequantized_stacks():
    T, H, I, E, top_k = 5, 128, 256, 4, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, H, generator=g).bfloat16()
    w_gu = (torch.randn(E, 2 * I, H, generator=g) / H**0.5).bfloat16()
    w_dn = (torch.randn(E, H, I, generator=g) / I**0.5).bfloat16()
    wts, ids = torch.topk(
        torch.softmax(torch.randn(T, E, generator=g), dim=-1), top_k, dim=-1
    )
    gu = ops.int4_quantize_experts(w_gu)
    dn = ops.int4_quantize_experts(w_dn)
    # the stacked triple is int4_quantize_weight of the [E*N, K] view
    flat = ops.int4_quantize_weight(w_gu.view(E * 2 * I, H))
    assert all(torch.equal(a.view(b.shape), b) for a, b in zip(gu, flat))
    deq_gu, deq_dn = (
        torch.stack([reference.int4_dequant(p[e], s[e], z[e])
                     for e in range(E)])
        for p, s, z in (gu, dn)
    )
    want = reference.fused_moe(x, deq_gu, deq_dn, ids, wts)
    assert torch.equal(ops.fused_moe_int4(x, gu, dn, ids, wts), want)


@pytest.mark.parametrize(
    "shape,ok",  # H, then I, 64- but not 128-aligned; P = 1026
    [((16, 2, 4, 512, 1024), True), ((16, 2, 4, 192, 1024), False),
     ((16, 2, 4, 512, 192), False), ((513, 2, 4, 512, 1024), False)],
)
def test_supported_truth_table(shape, ok):
    assert ops.fused_moe_int4_supported(*shape) is ok


def test_mini_mixtral_int4_engine():
    cfg = config.EngineConfig(
        model="mini-mixtral", max_model_len=256, quantization="int4",
        cache=config.CacheConfig(num_gpu_blocks=64, block_size=16),
        scheduler=config.SchedulerConfig(max_num_seqs=4,
                                         max_num_batched_tokens=256),
    )
    eng = LLMEngine(cfg, device="cpu")
    E, H, I = 4, 512, 1024
    shapes = {"experts_gate_up": (2 * I, H), "experts_down": (H, I)}
    for layer in eng.runner.model.layers:
        assert set(layer.int4_w) == {"qkv", "o", *shapes}
        for key, (N, K) in shapes.items():
            packed, s, z = layer.int4_w[key]
            assert (packed.dtype, s.dtype, z.dtype) == (
                torch.uint8, torch.bfloat16, torch.uint8)
            assert packed.shape == (E, N, K // 2)
            assert s.shape == z.shape == (E, N, K // 128)
            assert getattr(layer, key).numel() == 0
    params = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    out = eng.generate([list(range(20, 60))], params)["offline-0"]
    assert len(out) == 4
