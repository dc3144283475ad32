"""mini-llama served with quantization="fp8", fp8_gemm="native": every dense
projection of a step runs csrc/skinny_gemm_fp8.hip behind a fused act-quant
kernel, inside the captured decode hipGraphs."""

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

pytestmark = pytest.mark.gpu

PROMPT = list(range(50, 120))
PARAMS = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)


def _config(**kw):
    return EngineConfig(
        model="mini-llama",
        max_model_len=1024,
        cache=CacheConfig(num_gpu_blocks=256, block_size=16),
        scheduler=SchedulerConfig(max_num_seqs=16,
                                  max_num_batched_tokens=2048),
        quantization="fp8",
        fp8_gemm="native",
        **kw,
    )


@pytest.fixture(scope="module")
def graph_run():
    eng = LLMEngine(_config(), device="cuda")
    out = eng.generate([PROMPT], PARAMS)["offline-0"]
    return eng, out


def test_graphs_and_channel_scales(graph_run):
    eng, out = graph_run
    assert eng.runner.graphs is not None
    assert len(out) == 8
    for layer in eng.runner.model.layers:
        assert layer.fp8_gemm == "native"
        assert set(layer.fp8_w) == {"qkv", "o", "gate_up", "down"}
        for wq, sc in layer.fp8_w.values():
            assert wq.dtype == torch.float8_e4m3fn
            assert sc.dtype == torch.float32
            assert sc.shape == (wq.shape[0],)


def test_graph_matches_eager_and_counts_kernel(graph_run, monkeypatch):
    """Same seed, enforce_eager=True: token-identical to the graph engine
    (a row's GEMM result does not depend on the padded batch of a captured
    bucket), and every step runs the native kernel for its four projections
    in every layer."""
    _, out_graph = graph_run
    eager = LLMEngine(_config(enforce_eager=True), device="cuda")
    assert eager.runner.graphs is None
    layers = len(eager.runner.model.layers)

    calls = []
    real = ops.skinny_gemm_fp8

    def shim(*a):
        calls.append(a[0].shape[0])
        return real(*a)

    monkeypatch.setattr(ops, "skinny_gemm_fp8", shim)
    eager.add_request("r", PROMPT, PARAMS)
    out, per_step = [], []
    while eager.has_unfinished():
        del calls[:]
        for o in eager.step():
            if o.request_id == "r":
                out.extend(o.new_token_ids)
        per_step.append(list(calls))
    assert out == out_graph, (out, out_graph)
    assert len(per_step[0]) == 4 * layers and set(per_step[0]) == {len(PROMPT)}
    decode = per_step[1:]
    assert len(decode) == len(out) - 1  # the prefill step samples token 0
    for c in decode:
        assert len(c) == 4 * layers and set(c) == {1}, per_step


def test_matches_cpu_reference_engine(graph_run):
    """The project's criterion for fp8 serving
    (test_engine_gpu.test_fp8_weight_quantization_gpu): against a CPU engine
    rebuilt from the same quantized tensors, at least 2 of the first 4
    greedy tokens agree."""
    eng, out = graph_run
    cpu = LLMEngine(_config(), device="cpu")
    for lg, lc in zip(eng.runner.model.layers, cpu.runner.model.layers):
        lc.fp8_w = {
            k: (wq.cpu(), sc.cpu()) for k, (wq, sc) in lg.fp8_w.items()
        }
        lc.input_norm.data = lg.input_norm.data.cpu()
        lc.post_attn_norm.data = lg.post_attn_norm.data.cpu()
    cpu.runner.model.embed.data = eng.runner.model.embed.data.cpu()
    cpu.runner.model.final_norm.data = (
        eng.runner.model.final_norm.data.cpu()
    )
    cpu.runner.model.lm_head.data = eng.runner.model.lm_head.data.cpu()
    want = cpu.generate([PROMPT], PARAMS)["offline-0"]
    agree = sum(a == b for a, b in zip(out[:4], want[:4]))
    assert agree >= 2, (out, want)
