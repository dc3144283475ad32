"""EngineConfig.sampler = "native" end to end on the CPU, where ops.sample runs
reference.sample (the HIP kernel's contract in torch)."""

import pytest

from production_stack_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.sampling import SamplingParams

PROMPTS = [[1, 2, 3, 4, 5], [9, 8, 7]]


def generate(params, sampler="native", async_scheduling=False):
    cfg = EngineConfig(
        model="tiny-llama",
        max_model_len=256,
        seed=5,
        sampler=sampler,
        async_scheduling=async_scheduling,
        cache=CacheConfig(num_gpu_blocks=128, block_size=16),
        scheduler=SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=128),
    )
    eng = LLMEngine(cfg, device="cpu")
    out = eng.generate(PROMPTS, params)
    return [out[f"offline-{i}"] for i in range(len(PROMPTS))], eng


def stochastic(seed):
    return SamplingParams(max_tokens=8, temperature=0.8, top_p=0.9, top_k=40,
                          min_p=0.01, seed=seed, ignore_eos=True)


def test_seeded_request_repeats_and_seed_matters():
    a, _ = generate(stochastic(7))
    b, _ = generate(stochastic(7))
    c, _ = generate(stochastic(8))
    assert a == b
    assert a != c
    assert all(len(t) == 8 for t in a)


def test_seeded_request_same_tokens_sync_and_async():
    """A seeded row's counter is its output length, placeholders included, so
    the one-step-lagged path draws what the synchronous one does, and it
    stays on the async path."""
    want, _ = generate(stochastic(7))
    got, eng = generate(stochastic(7), async_scheduling=True)
    assert got == want
    assert eng.runner.async_steps >= 8


def test_top_k_1_is_greedy():
    greedy = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    top1 = SamplingParams(max_tokens=8, temperature=1.0, top_k=1,
                          ignore_eos=True)
    assert generate(top1)[0] == generate(greedy)[0]


def test_unknown_sampler_raises():
    with pytest.raises(ValueError, match="sampler"):
        generate(SamplingParams(max_tokens=1), sampler="bogus")
