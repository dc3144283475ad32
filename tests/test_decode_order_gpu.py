"""GPU tests of the longest-first decode launch order and of the pipelined
decode kernel (variant 2). Neither may change a single output bit, so the
comparisons are torch.equal; only the check against the fp32 reference uses
the tolerance of tests/test_kernels_gpu.py::test_paged_attn_decode."""

import functools

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.ops import reference

pytestmark = pytest.mark.gpu

BS = 16
CTX_CHOICES = [1, 15, 16, 17, 63, 64, 65, 300]
MAX_BLOCKS = (300 + BS - 1) // BS + 2
HEADS = [(32, 8, 128), (8, 8, 128), (4, 4, 64)]


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


@pytest.mark.parametrize("S", [1, 2, 7, 64, 65, 640])
def test_decode_order_is_stable_descending_argsort(S):
    g = torch.Generator().manual_seed(S)
    choices = torch.tensor([1, 16, 17, 300], dtype=torch.int32)
    lens = choices[torch.randint(0, 4, (S,), generator=g)]
    got = ops.decode_order(lens.cuda())
    want = torch.argsort(lens, descending=True, stable=True)
    assert got.dtype == torch.int32
    assert torch.equal(got.cpu().long(), want)


def test_decode_order_over_the_cap_is_unsupported():
    lens = torch.ones(4097, dtype=torch.int32, device="cuda")
    assert ops.decode_order(lens) is None


@functools.lru_cache(maxsize=None)
def _case(S, qh, kh, hd, fp8=False):
    """One seeded problem per shape, shared by the tests below: contexts of
    1-19 blocks (some of the 4 waves get no block; single valid tokens in a
    last block), shuffled non-contiguous block tables."""
    g = torch.Generator().manual_seed(1000 * S + qh + hd)
    lens = torch.tensor(CTX_CHOICES, dtype=torch.int32)[
        torch.randint(0, len(CTX_CHOICES), (S,), generator=g)]
    lens[:len(CTX_CHOICES)] = torch.tensor(
        CTX_CHOICES, dtype=torch.int32)[:S][torch.randperm(
            min(S, len(CTX_CHOICES)), generator=g)]
    nb = S * MAX_BLOCKS + 1
    k = torch.randn((nb, kh, BS, hd), generator=g).to(torch.bfloat16)
    v = torch.randn((nb, kh, BS, hd), generator=g).to(torch.bfloat16)
    if fp8:
        k = k.to(torch.float8_e4m3fn)
        v = v.to(torch.float8_e4m3fn)
    bt = (torch.randperm(S * MAX_BLOCKS, generator=g) + 1).to(
        torch.int32).reshape(S, MAX_BLOCKS)
    q = torch.randn((S, qh, hd), generator=g).to(torch.bfloat16)
    return dict(q=q.cuda(), k=k.cuda(), v=v.cuda(), bt=bt.cuda(),
                lens=lens.cuda(), scale=1.0 / hd ** 0.5,
                perm=torch.randperm(S, generator=g).int().cuda())


def _run(c, variant, order=None, num_splits=1, window=0):
    from production_stack_amd import _C

    out = torch.full_like(c["q"], float("nan"))
    _C.paged_attn_decode(out, c["q"], c["k"], c["v"], c["bt"], c["lens"],
                         c["scale"], num_splits, variant, window, order)
    return out


def _orders(c):
    return [ops.decode_order(c["lens"]), c["perm"]]


CONFIGS = [(S, h, ns, 0, False)
           for S in (5, 37) for h in HEADS for ns in (1, 3)]
CONFIGS += [(37, HEADS[0], 1, 40, False), (5, HEADS[0], 3, 40, False),
            (37, HEADS[0], 1, 0, True), (5, HEADS[0], 3, 0, True)]


@pytest.mark.parametrize("S,heads,num_splits,window,fp8", CONFIGS)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_order_is_invisible(S, heads, num_splits, window, fp8, variant):
    c = _case(S, *heads, fp8=fp8)
    base = _run(c, variant, None, num_splits, window)
    assert not torch.isnan(base.float()).any()
    for order in _orders(c):
        got = _run(c, variant, order, num_splits, window)
        assert torch.equal(got, base)


@pytest.mark.parametrize("S,heads,num_splits,window,fp8", CONFIGS)
def test_variant2_equals_variant1(S, heads, num_splits, window, fp8):
    c = _case(S, *heads, fp8=fp8)
    for order in [None] + _orders(c):
        v1 = _run(c, 1, order, num_splits, window)
        v2 = _run(c, 2, order, num_splits, window)
        assert torch.equal(v2, v1)


@pytest.mark.parametrize("heads", HEADS)
def test_variant2_matches_reference(heads):
    c = _case(37, *heads)
    want = reference.paged_attn_decode(
        c["q"].cpu(), c["k"].cpu(), c["v"].cpu(), c["bt"].cpu(),
        c["lens"].cpu(), c["scale"])
    for order in [None, ops.decode_order(c["lens"])]:
        got = _run(c, 2, order, 0)
        torch.testing.assert_close(got.float().cpu(), want.float().cpu(),
                                   atol=2e-2, rtol=2e-2)


def test_ops_default_matches_variant1():
    c = _case(37, *HEADS[0])
    got = ops.paged_attn_decode(c["q"], c["k"], c["v"], c["bt"], c["lens"],
                                c["scale"], 0, ops.decode_order(c["lens"]))
    assert torch.equal(got, _run(c, 1, None, 0))


def test_graph_replay_orders_by_live_seq_lens():
    """A captured decode forward must sort the seq_lens it is replayed with,
    not those it was captured with."""
    from production_stack_amd.engine.config import ModelConfig
    from production_stack_amd.engine.graph_runner import DecodeGraphRunner
    from production_stack_amd.engine.models.llama import LlamaForCausalLM

    cfg = ModelConfig(
        name="graph-order-test", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_q_heads=8, num_kv_heads=2,
        head_dim=128, max_position=512,
    )
    model = LlamaForCausalLM(cfg).cuda()
    model.random_init(seed=3)
    B, nb = 8, 8 * MAX_BLOCKS + 1
    g = torch.Generator().manual_seed(5)
    kv = [tuple(torch.randn((nb, 2, BS, 128), generator=g)
                .to(torch.bfloat16).cuda() for _ in range(2))
          for _ in range(cfg.num_layers)]
    runner = DecodeGraphRunner(model, kv, B, MAX_BLOCKS, torch.device("cuda"))

    def fill(lens, seed):
        gg = torch.Generator().manual_seed(seed)
        runner.tokens.copy_(torch.randint(0, 512, (B,), generator=gg))
        runner.seq_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        runner.positions.copy_(torch.tensor(lens, dtype=torch.int32) - 1)
        runner.block_tables.copy_(
            (torch.randperm(B * MAX_BLOCKS, generator=gg) + 1)
            .to(torch.int32).reshape(B, MAX_BLOCKS))
        # slots stay -1: no KV append, the caches are read-only here

    meta = runner._meta(B)  # one meta per bucket, as capture_all builds it
    fill([300, 1, 17, 64, 15, 65, 16, 63], seed=1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # warm up outside the capture
            model(runner.tokens[:B], meta, kv)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hidden = model(runner.tokens[:B], meta, kv)
    # new inputs whose length ranking differs from the captured one
    fill([1, 300, 63, 16, 65, 15, 64, 17], seed=2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = hidden.clone()
    want_order = ops.decode_order(runner.seq_lens[:B])
    assert torch.equal(meta.decode_order, want_order)
    eager = model(runner.tokens[:B], runner._meta(B), kv)
    assert torch.equal(replayed, eager)
