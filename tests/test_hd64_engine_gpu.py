"""A head_dim-64 Llama (8 q heads, 2 kv heads) served end to end: chunked
prefill with history, mixed steps and decode run the MFMA prefill kernel of
csrc/prefill_mfma64.hip, never the VALU prefill, with a bf16 and an fp8 KV
cache. Numerics are the op tests' business."""

import dataclasses

import pytest

from production_stack_amd import ops
from production_stack_amd.engine.config import (
    ARCHITECTURES,
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.sampling import SamplingParams

pytestmark = pytest.mark.gpu

SHORT = list(range(50, 70))
LONG = list(range(300, 500))  # three prefill chunks of at most 96 rows


@pytest.mark.parametrize("kv_cache_dtype", ["bf16", "fp8"])
def test_hd64_engine_prefills_on_mfma(kv_cache_dtype, monkeypatch):
    monkeypatch.setitem(
        ARCHITECTURES, "mini-llama-hd64",
        dataclasses.replace(ARCHITECTURES["mini-llama"], num_q_heads=8,
                            num_kv_heads=2, head_dim=64))
    eng = LLMEngine(EngineConfig(
        model="mini-llama-hd64",
        max_model_len=1024,
        cache=CacheConfig(num_gpu_blocks=256, block_size=16,
                          kv_cache_dtype=kv_cache_dtype),
        scheduler=SchedulerConfig(max_num_seqs=16,
                                  max_num_batched_tokens=2048,
                                  max_prefill_chunk=96),
        enforce_eager=True,
    ), device="cuda")
    layers = len(eng.runner.model.layers)
    mfma_rows = []
    real = ops.paged_attn_prefill_mfma

    def shim(q, *a, **kw):
        mfma_rows.append(q.shape[0])
        return real(q, *a, **kw)

    def valu(*a, **kw):
        raise AssertionError("VALU prefill ran at head_dim 64")

    monkeypatch.setattr(ops, "paged_attn_prefill_mfma", shim)
    monkeypatch.setattr(ops, "paged_attn_prefill", valu)
    params = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    done = {"short": [], "long": []}

    def step():
        for o in eng.step():
            done[o.request_id].extend(o.new_token_ids)

    eng.add_request("short", SHORT, params)
    step()  # the short request decodes while the long one prefills
    eng.add_request("long", LONG, dataclasses.replace(params))
    while eng.has_unfinished():
        step()
    assert len(done["short"]) == 8 and len(done["long"]) == 8, done
    assert sum(mfma_rows) == layers * (len(SHORT) + len(LONG)), mfma_rows
    assert max(mfma_rows) <= 96
