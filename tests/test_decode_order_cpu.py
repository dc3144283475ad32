"""CPU tests of the longest-first decode launch order: the op's fallback and
the model/engine plumbing (the order itself only matters to the GPU kernel)."""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.models import llama
from production_stack_amd.engine.sampling import SamplingParams


@pytest.mark.parametrize("S", [1, 2, 7, 64, 65, 640])
def test_decode_order_cpu_is_stable_descending_argsort(S):
    g = torch.Generator().manual_seed(S)
    choices = torch.tensor([1, 16, 17, 300], dtype=torch.int32)
    lens = choices[torch.randint(0, 4, (S,), generator=g)]
    got = ops.decode_order(lens)
    want = torch.argsort(lens, descending=True, stable=True)
    assert got.dtype == torch.int32
    assert torch.equal(got.long(), want)


def test_batch_meta_has_no_order_until_forward():
    meta = llama.BatchMeta(
        positions=torch.zeros(1, dtype=torch.int32),
        slot_mapping=torch.zeros(1, dtype=torch.long),
        num_prefill_tokens=0, prefill_token_seq=None,
        prefill_token_pos=None, prefill_block_tables=None,
        num_decode_seqs=1,
        decode_seq_lens=torch.ones(1, dtype=torch.int32),
        decode_block_tables=torch.zeros((1, 1), dtype=torch.int32),
    )
    assert meta.decode_order is None
    # CPU tensors: the forward asks for no order
    assert not llama._decode_order_wanted(meta)


_REAL_DECODE = ops.paged_attn_decode


def _generate(monkeypatch, with_order):
    seen = []
    real_decode = _REAL_DECODE

    def spy(q, k_cache, v_cache, block_tables, seq_lens, scale, window=0,
            order=None):
        seen.append((order, seq_lens.clone()))
        return real_decode(q, k_cache, v_cache, block_tables, seq_lens,
                           scale, window, order)

    monkeypatch.setattr(ops, "paged_attn_decode", spy)
    if with_order:
        monkeypatch.setattr(
            llama, "_decode_order_wanted",
            lambda meta: meta.num_decode_seqs > 0,
        )
    cfg = EngineConfig(
        model="tiny-llama",
        max_model_len=256,
        cache=CacheConfig(num_gpu_blocks=128, block_size=16),
        # 32-token budget: the 80-token prompt prefills in chunks while the
        # short prompts already decode (mixed steps)
        scheduler=SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=32),
    )
    eng = LLMEngine(cfg, device="cpu")
    prompts = [list(range(10, 90)), [7, 8, 9], list(range(200, 230)),
               [5, 6]]
    out = eng.generate(
        prompts, SamplingParams(max_tokens=6, temperature=0.0,
                                ignore_eos=True))
    return out, seen


def test_engine_tokens_do_not_depend_on_decode_order(monkeypatch):
    base, seen0 = _generate(monkeypatch, with_order=False)
    assert seen0 and all(o is None for o, _ in seen0)
    with_order, seen1 = _generate(monkeypatch, with_order=True)
    assert with_order == base
    assert len(seen1) == len(seen0)
    multi = 0
    for order, lens in seen1:
        # every decode call got the order of ITS seq_lens
        assert order is not None and order.dtype == torch.int32
        assert torch.equal(
            order.long(), torch.argsort(lens, descending=True, stable=True))
        multi += int(lens.numel() > 1 and lens.unique().numel() > 1)
    assert multi > 0, "no ragged multi-sequence decode step was exercised"
