"""ops.sample (csrc/sample.hip) against its contract in float64.

The pick is checked with explicit uniforms: for a row's kept set and CDF in
token-id order, computed in float64 from the contract, every kept token whose
interval is wider than 1e-3 (the 64 widest at most) gets u = the interval's
midpoint and must come back exactly. A midpoint is more than 5e-4 from either
boundary, against the kernel's fp32 / 2^-40 fixed-point error of order 1e-6,
so there is no tolerance.
"""

import math

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.ops import reference

pytestmark = pytest.mark.gpu

NONE = (1.0, -1, 1.0, 0.0)
TOP_K = (0.7, 50, 1.0, 0.0)
TOP_P = (1.0, -1, 0.9, 0.0)
MIN_P = (1.5, -1, 1.0, 0.05)
ALL = (0.8, 40, 0.9, 0.02)
TOP_1 = (1.0, 1, 1.0, 0.0)
K_GE_V = (1.0, 1 << 20, 0.95, 0.0)
GREEDY = (0.0, 5, 0.5, 0.5)


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def pack(tuples, key=None, counter=None):
    n = len(tuples)
    t, k, p, m = zip(*tuples)
    return ops.sample_pack(t, k, p, m, key or [0] * n, counter or [0] * n)


def contract_cdf(x, T, top_k, top_p, min_p):
    """The kept set's normalised CDF in token-id order, float64."""
    x = x.double()
    V = x.numel()
    T, top_p, min_p = f32(T), f32(top_p), f32(min_p)
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        keep &= x >= torch.sort(x, descending=True).values[top_k - 1]
    d = x / T - (x / T).max()
    if min_p > 0:
        keep &= d >= math.log(min_p)
    p = torch.exp(d) * keep
    if top_p < 1:
        sp = torch.sort(p[keep], descending=True).values
        before = torch.cumsum(sp, 0) - sp
        b = int((before / sp.sum() < top_p).nonzero()[-1])
        keep &= p >= sp[b]
    p = p * keep
    return torch.cumsum(p, 0) / p.sum()


def midpoints(cdf):
    """[(token, u)] for the (at most 64) widest intervals wider than 1e-3."""
    lo = torch.cat([torch.zeros(1, dtype=cdf.dtype), cdf[:-1]])
    width = cdf - lo
    order = torch.argsort(width, descending=True)[:64]
    return [(int(i), float((lo[i] + cdf[i]) / 2)) for i in order
            if width[i] > 1e-3]


def check_picks(logits, tuples):
    R = logits.shape[0]
    want = []
    for r, tup in enumerate(tuples):
        if tup[0] == 0.0:  # argmax whatever u is
            want.append([(int(logits[r].double().argmax()), 0.5)])
        else:
            want.append(midpoints(contract_cdf(logits[r], *tup)))
        assert want[r], f"row {r}: nothing to check"
    dev, params = logits.cuda(), pack(tuples).cuda()
    n = max(len(w) for w in want)
    got = torch.stack([
        ops.sample(dev, params, u=torch.tensor(
            [want[r][j % len(want[r])][1] for r in range(R)],
            dtype=torch.float32, device="cuda"))
        for j in range(n)
    ]).cpu()
    for r in range(R):
        for j in range(n):
            tok, u = want[r][j % len(want[r])]
            assert int(got[j, r]) == tok, (
                f"row {r} {tuples[r]} u={u}: got {int(got[j, r])}, "
                f"want {tok}")
    print(f"checked {sum(len(w) for w in want)} picks")


@pytest.mark.parametrize("V", [8, 1000, 1001, 4104, 152064])
@pytest.mark.parametrize("tuples", [
    (NONE, TOP_K, TOP_P), (MIN_P, ALL, TOP_1), (K_GE_V, GREEDY, ALL),
], ids=["none-topk-topp", "minp-all-top1", "kgev-greedy-all"])
def test_pick_matches_contract(V, tuples):
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(3, V, generator=g) * 4).to(torch.bfloat16)
    check_picks(logits, tuples)


def test_tie_class_stays_whole_at_the_boundaries():
    """20 equal logits straddle both the 10th-largest position and the
    top_p = 0.7 mass boundary: all 20 stay, under top-k, top-p and both."""
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(3, 1000, generator=g).to(torch.bfloat16)
    logits[:, 5:8] = torch.tensor([8.0, 7.5, 7.0], dtype=torch.bfloat16)
    logits[:, 100:120] = 6.0
    tuples = ((1.0, 10, 1.0, 0.0), (1.0, -1, 0.7, 0.0), (1.0, 10, 0.7, 0.0))
    for r, tup in enumerate(tuples):
        cdf = contract_cdf(logits[r], *tup)
        kept = {t for t, _ in midpoints(cdf)}
        assert set(range(100, 120)) <= kept
    check_picks(logits, tuples)


def test_philox_uniform():
    # Philox4x32-10 known answer, counter = key = 0: word 0 is 0x6627e8d5
    assert reference.philox_uniform(0, 0) == 0x6627E8 * 2.0 ** -24
    keys = [0, (1 << 32) + 5, (1 << 63) + 12345, 42, 7]
    ctrs = [0, 1 << 32, 7, (1 << 40) + 3, (1 << 32) - 1]
    logits = torch.zeros(5, 16, dtype=torch.bfloat16, device="cuda")
    _, u = ops.sample(logits, pack([NONE] * 5, keys, ctrs), return_u=True)
    want = [reference.philox_uniform(k, c) for k, c in zip(keys, ctrs)]
    assert u.cpu().double().tolist() == want
    assert len(set(want)) == 5


def test_temperature_zero_is_greedy_sample():
    g = torch.Generator().manual_seed(2)
    logits = (torch.randn(4, 4104, generator=g) * 4).to(torch.bfloat16)
    logits[1] = 1.5  # all equal: index 0
    logits[2, 77] = logits[2, 3000] = 30.0  # tied maxima: the first
    dev = logits.cuda()
    got = ops.sample(dev, pack([GREEDY] * 4))
    assert torch.equal(got, ops.greedy_sample(dev))
    assert got.cpu().tolist()[1:3] == [0, 77]


def test_deterministic_and_row_independent():
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(3, 4104, generator=g) * 4).to(torch.bfloat16).cuda()
    tuples, keys, ctrs = [NONE, ALL, TOP_P], [11, 12, 13], [5, 6, 1 << 32]
    a = ops.sample(logits, pack(tuples, keys, ctrs))
    b = ops.sample(logits, pack(tuples, keys, ctrs))
    assert torch.equal(a, b)
    for r in range(3):
        one = ops.sample(logits[r:r + 1],
                         pack(tuples[r:r + 1], keys[r:r + 1], ctrs[r:r + 1]))
        assert int(one) == int(a[r])


@pytest.mark.parametrize("dtype, tup", [
    (torch.float32, NONE),
    (torch.bfloat16, (1.0, -1, 0.0, 0.0)),
    (torch.bfloat16, (-1.0, -1, 1.0, 0.0)),
    (torch.bfloat16, (1.0, -1, 1.0, 1.5)),
], ids=["fp32-logits", "top_p-0", "negative-temperature", "min_p-above-1"])
def test_rejections(dtype, tup):
    logits = torch.zeros(2, 64, dtype=dtype, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        ops.sample(logits, pack([tup] * 2))
    torch.cuda.synchronize()


def test_engine_mixed_batch_stays_async():
    """Greedy and seeded stochastic requests in one async-scheduled batch:
    completes, repeats, and no step leaves the one-step-lagged path for
    sampling."""
    from production_stack_amd.engine.config import (
        CacheConfig,
        EngineConfig,
        SchedulerConfig,
    )
    from production_stack_amd.engine.engine import LLMEngine
    from production_stack_amd.engine.sampling import SamplingParams

    def run():
        cfg = EngineConfig(
            model="mini-llama", max_model_len=512, seed=3,
            enforce_eager=True, async_scheduling=True, sampler="native",
            cache=CacheConfig(num_gpu_blocks=64, block_size=16),
            scheduler=SchedulerConfig(max_num_seqs=8,
                                      max_num_batched_tokens=256),
        )
        eng = LLMEngine(cfg, device="cuda")
        params = [
            SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
            if i % 2 == 0 else
            SamplingParams(max_tokens=12, temperature=0.8, top_p=0.9,
                           seed=100 + i, ignore_eos=True)
            for i in range(4)
        ]
        prompts = [[(7 * i + j) % 2000 + 5 for j in range(20)]
                   for i in range(4)]
        out = eng.generate(prompts, params)
        return [out[f"offline-{i}"] for i in range(4)], eng.runner.async_steps

    a, steps_a = run()
    b, _ = run()
    assert all(len(t) == 12 for t in a)
    assert a == b
    assert steps_a >= 12  # prefill + 11 decode steps, none synchronous
