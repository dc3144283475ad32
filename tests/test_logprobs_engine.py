"""Logprobs under EngineConfig.sampler = "native", on the CPU, where
ops.logprobs runs reference.logprobs (csrc/logprobs.hip's contract in torch)."""

import pytest

from production_stack_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.sampling import SamplingParams

PROMPTS = [[1, 2, 3, 4, 5], [9, 8, 7]]
MAX_TOKENS = 8


def run(params, sampler="native", async_scheduling=False):
    """Per prompt: tokens, their logprobs, their alternatives, prompt
    logprobs; and the engine."""
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
    for i, p in enumerate(PROMPTS):
        eng.add_request(f"r{i}", p, params)
    got = {f"r{i}": ([], [], [], []) for i in range(len(PROMPTS))}
    while eng.has_unfinished():
        for r in eng.step():
            toks, lps, tops, plp = got[r.request_id]
            toks.extend(r.new_token_ids)
            lps.extend(r.new_logprobs or [])
            tops.extend(r.new_top_logprobs or [])
            plp.extend(r.prompt_logprobs or [])
    return [got[f"r{i}"] for i in range(len(PROMPTS))], eng


def test_logprobs_stay_on_the_async_path_and_match_sync():
    params = SamplingParams(max_tokens=MAX_TOKENS, temperature=0.8, top_p=0.9,
                            top_k=40, seed=7, logprobs=5, ignore_eos=True)
    want, _ = run(params)
    got, eng = run(params, async_scheduling=True)
    assert eng.runner.async_steps >= MAX_TOKENS
    assert not eng.runner.last_logprobs and not eng.runner.last_top_logprobs
    for (wt, wl, wa, _), (gt, gl, ga, _) in zip(want, got):
        assert gt == wt and len(gt) == MAX_TOKENS
        assert gl == wl and len(gl) == MAX_TOKENS
        assert ga == wa and all(len(a) == 5 for a in ga)


@pytest.mark.parametrize("async_scheduling", [False, True])
def test_greedy_token_is_the_first_alternative(async_scheduling):
    params = SamplingParams(max_tokens=MAX_TOKENS, temperature=0.0,
                            logprobs=3, ignore_eos=True)
    got, eng = run(params, async_scheduling=async_scheduling)
    assert eng.runner.async_steps >= (MAX_TOKENS if async_scheduling else 0)
    for toks, lps, tops, _ in got:
        assert len(toks) == len(lps) == len(tops) == MAX_TOKENS
        for tok, lp, alts in zip(toks, lps, tops):
            assert alts[0] == (tok, lp)
            vals = [v for _, v in alts]
            assert vals == sorted(vals, reverse=True)


def test_prompt_logprobs_match_the_torch_sampler():
    params = SamplingParams(max_tokens=2, temperature=0.0, prompt_logprobs=0,
                            ignore_eos=True)
    want, _ = run(params, sampler="torch")
    got, _ = run(params)
    for prompt, (_, _, _, w), (_, _, _, g) in zip(PROMPTS, want, got):
        assert len(g) == len(w) == len(prompt) and g[0] is None
        assert g[1:] == pytest.approx(w[1:], abs=1e-4)
