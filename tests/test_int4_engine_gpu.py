"""mini-llama served with quantization="int4": every dense projection of a
decode step runs csrc/skinny_gemm_w4.hip on bf16 activations, inside the
captured decode hipGraphs; prefill chunks above the kernel's M range
dequantize into a transient bf16 buffer; LoRA stays available."""

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
KEYS = {"qkv", "o", "gate_up", "down"}


def _config(**kw):
    return EngineConfig(
        model="mini-llama",
        max_model_len=1024,
        cache=CacheConfig(num_gpu_blocks=256, block_size=16),
        scheduler=SchedulerConfig(max_num_seqs=16,
                                  max_num_batched_tokens=2048),
        quantization="int4",
        **kw,
    )


@pytest.fixture(scope="module")
def graph_run():
    eng = LLMEngine(_config(), device="cuda")
    out = eng.generate([PROMPT], PARAMS)["offline-0"]
    return eng, out


@pytest.fixture(scope="module")
def eager():
    eng = LLMEngine(_config(enforce_eager=True), device="cuda")
    assert eng.runner.graphs is None
    return eng


def _count(monkeypatch):
    """Wrap the two int4 kernels' entry points; returns (gemm Ms, dequant
    shapes), filled as they are called."""
    gemm, deq = [], []
    real_gemm, real_deq = ops.skinny_gemm_w4, ops.int4_dequant

    def gemm_shim(*a):
        gemm.append(a[0].shape[0])
        return real_gemm(*a)

    def deq_shim(*a):
        deq.append(tuple(a[0].shape))
        return real_deq(*a)

    monkeypatch.setattr(ops, "skinny_gemm_w4", gemm_shim)
    monkeypatch.setattr(ops, "int4_dequant", deq_shim)
    return gemm, deq


def _steps(eng, rid, prompt, gemm, deq):
    eng.add_request(rid, prompt, PARAMS)
    out, per_step = [], []
    while eng.has_unfinished():
        del gemm[:], deq[:]
        for o in eng.step():
            if o.request_id == rid:
                out.extend(o.new_token_ids)
        per_step.append((list(gemm), list(deq)))
    return out, per_step


def test_graphs_and_layout(graph_run):
    eng, out = graph_run
    assert eng.runner.graphs is not None
    assert len(out) == 8
    shapes = {
        "qkv": (1024, 512), "o": (512, 512),
        "gate_up": (2048, 512), "down": (512, 1024),
    }
    for layer in eng.runner.model.layers:
        assert set(layer.int4_w) == KEYS
        for key, (packed, s, z) in layer.int4_w.items():
            N, K = shapes[key]
            assert packed.dtype == torch.uint8 and packed.shape == (N, K // 2)
            assert s.dtype == torch.bfloat16 and s.shape == (N, K // 128)
            assert z.dtype == torch.uint8 and z.shape == (N, K // 128)
            assert packed.is_cuda and s.is_cuda and z.is_cuda
        for pname in ("qkv_proj", "o_proj", "gate_up_proj", "down_proj"):
            assert getattr(layer, pname).numel() == 0, pname


def test_graph_matches_eager_and_counts_kernel(graph_run, eager, monkeypatch):
    """Same seed, enforce_eager=True: token-identical to the graph engine
    (a row's GEMM result does not depend on the padded batch of a captured
    bucket), and every step runs the native kernel for its four projections
    in every layer."""
    _, out_graph = graph_run
    layers = len(eager.runner.model.layers)
    gemm, deq = _count(monkeypatch)
    out, per_step = _steps(eager, "short", PROMPT, gemm, deq)
    assert out == out_graph, (out, out_graph)
    g0, d0 = per_step[0]
    assert len(g0) == 4 * layers and set(g0) == {len(PROMPT)} and d0 == []
    decode = per_step[1:]
    assert len(decode) == len(out) - 1  # the prefill step samples token 0
    for g, d in decode:
        assert len(g) == 4 * layers and set(g) == {1} and d == [], per_step


def test_long_prefill_dequantizes(eager, monkeypatch):
    """A 300-token prefill step is above the kernel's M range: no native
    GEMM call, one int4_dequant per projection per layer, and generation
    completes."""
    layers = len(eager.runner.model.layers)
    gemm, deq = _count(monkeypatch)
    out, per_step = _steps(eager, "long", list(range(40, 340)), gemm, deq)
    g0, d0 = per_step[0]
    assert g0 == [] and len(d0) == 4 * layers, per_step[0]
    assert len(out) == 8
    for g, d in per_step[1:]:
        assert len(g) == 4 * layers and set(g) == {1} and d == []


def test_matches_cpu_reference_engine(graph_run):
    """The project's criterion for quantized serving
    (test_fp8_native_engine_gpu.test_matches_cpu_reference_engine): against
    a CPU engine rebuilt from the same quantized tensors, at least 2 of the
    first 4 greedy tokens agree."""
    eng, out = graph_run
    cpu = LLMEngine(_config(), device="cpu")
    for lg, lc in zip(eng.runner.model.layers, cpu.runner.model.layers):
        lc.int4_w = {
            k: tuple(t.cpu() for t in v) for k, v in lg.int4_w.items()
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


def test_int4_with_lora(tmp_path):
    """Activations stay bf16, so the LoRA slot path runs on top of int4
    weights inside the captured graphs (the fp8 fused path has to switch
    LoRA off)."""
    from production_stack_amd.engine.lora import save_synthetic_adapter

    adir = str(tmp_path / "ad")
    save_synthetic_adapter(adir, hidden=512, q_size=512, kv_size=256,
                           num_layers=4, seed=9)
    eng = LLMEngine(_config(enable_lora=True, max_loras=2, max_lora_rank=8),
                    device="cuda")
    assert eng.runner.graphs is not None and eng.runner.graphs.use_lora
    assert all(set(l.int4_w) == KEYS for l in eng.runner.model.layers)
    eng.load_lora("ad", adir)
    prompt = list(range(300, 340))
    eng.add_request("base", prompt, PARAMS)
    eng.add_request("lora", prompt, PARAMS, lora_name="ad")
    outs = {"base": [], "lora": []}
    while eng.has_unfinished():
        for r in eng.step():
            outs[r.request_id].extend(r.new_token_ids)
    assert len(outs["base"]) == 8 and len(outs["lora"]) == 8
    assert outs["base"] != outs["lora"], "adapter must change the tokens"
