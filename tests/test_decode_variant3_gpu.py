"""GPU tests of decode variant 3 (next K tile prefetched, score reduction in
DPP) and of the `out=` argument of the two attention ops.

Variant 3 performs variant 2's floating-point operations in the same order,
so it must equal variant 2 bit for bit. Both are also held to the same
yardstick: reference.paged_attn_decode on the CPU on float64 copies of the
same bf16 inputs, so that its result is not rounded to bf16 (the reference's
own arithmetic is fp32 on these exactly representable inputs; its error,
~1e-6 relative, is three orders below one bf16 output ulp). The tolerance is
that of tests/test_kernels_gpu.py::test_paged_attn_decode (atol = rtol =
2e-2). Every call forces its variant; none depends on ops.DECODE_VARIANT.

Unused block-table entries point at a poison block of NaNs that no live
entry uses: a row read past a sequence's last block, and used, shows as NaN
in the output without the read leaving the cache allocation."""

import functools
import math

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.ops import reference

pytestmark = pytest.mark.gpu

BS = 16
KH = 2
NB = 64            # usable cache blocks; block NB is the poison block
MAX_BLOCKS = 24
TOL = dict(atol=2e-2, rtol=2e-2)
# every (head_dim, GQ) the dispatcher instantiates
GROUPS = [(128, g) for g in (1, 2, 3, 4, 6, 7, 8)] + \
         [(64, g) for g in (1, 2, 4, 8)]
# a lone token, the block edges, a partial last block with masked rows
CTX_BATCHES = [(1, 16, 100), (15, 17, 33)]


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


@functools.lru_cache(maxsize=None)
def _case(hd, gq, lens, peaked=False):
    """One seeded problem per shape, shared by the tests and never modified:
    block tables are a shuffled, non-contiguous subset of the cache."""
    S = len(lens)
    g = torch.Generator().manual_seed(7919 * hd + 31 * gq + sum(lens))
    k = torch.randn((NB + 1, KH, BS, hd), generator=g)
    v = torch.randn((NB + 1, KH, BS, hd), generator=g)
    bt = torch.full((S, MAX_BLOCKS), NB, dtype=torch.int32)
    perm = torch.randperm(NB, generator=g).to(torch.int32)
    used = 0
    for s, n in enumerate(lens):
        nblk = (n + BS - 1) // BS
        bt[s, :nblk] = perm[used:used + nblk]
        used += nblk
        if peaked:
            # first and last key x8: a peaked softmax whose running max
            # moves again in the last block
            k[int(bt[s, 0]), :, 0] *= 8.0
            k[int(bt[s, nblk - 1]), :, (n - 1) % BS] *= 8.0
    k[NB] = float("nan")
    v[NB] = float("nan")
    k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
    q = torch.randn((S, KH * gq, hd), generator=g).to(torch.bfloat16)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    c = dict(q=q.cuda(), k=k.cuda(), v=v.cuda(), bt=bt.cuda(),
             lens=lens_t.cuda(), scale=1.0 / hd ** 0.5,
             cpu=(q, k, v, bt, lens_t))
    return c


@functools.lru_cache(maxsize=None)
def _want(hd, gq, lens, peaked=False, window=0):
    q, k, v, bt, lens_t = _case(hd, gq, lens, peaked)["cpu"]
    return reference.paged_attn_decode(
        q.double(), k.double(), v.double(), bt, lens_t,
        1.0 / hd ** 0.5, window)


def _run(c, variant, order=None, num_splits=1, window=0):
    from production_stack_amd import _C

    out = torch.full_like(c["q"], float("nan"))
    _C.paged_attn_decode(out, c["q"], c["k"], c["v"], c["bt"], c["lens"],
                         c["scale"], num_splits, variant, window, order)
    return out


def _errors(got, want):
    err = (got.double().cpu() - want).abs()
    return float(err.max()), float(err.mean())


def _bf16_ulp(x):
    """One bf16 ulp (8 significand bits) at magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 7)


@pytest.mark.parametrize("lens", CTX_BATCHES)
@pytest.mark.parametrize("hd,gq", GROUPS)
def test_variant3_accuracy(hd, gq, lens):
    c = _case(hd, gq, lens)
    want = _want(hd, gq, lens)
    got3, got2 = _run(c, 3), _run(c, 2)
    e3, e2 = _errors(got3, want), _errors(got2, want)
    print(f"hd={hd} gq={gq} lens={lens}: v3 max/mean {e3[0]:.3e}/{e3[1]:.3e}"
          f"  v2 max/mean {e2[0]:.3e}/{e2[1]:.3e}")
    torch.testing.assert_close(got3.double().cpu(), want, **TOL)
    assert e3[0] <= e2[0] + _bf16_ulp(float(want.abs().max()))
    assert torch.equal(got3, got2)


@pytest.mark.parametrize("lens", CTX_BATCHES)
def test_variant3_accuracy_peaked_softmax(lens):
    c = _case(128, 4, lens, peaked=True)
    want = _want(128, 4, lens, peaked=True)
    got3, got2 = _run(c, 3), _run(c, 2)
    e3, e2 = _errors(got3, want), _errors(got2, want)
    print(f"peaked lens={lens}: v3 max/mean {e3[0]:.3e}/{e3[1]:.3e}"
          f"  v2 max/mean {e2[0]:.3e}/{e2[1]:.3e}")
    torch.testing.assert_close(got3.double().cpu(), want, **TOL)
    assert e3[0] <= e2[0] + _bf16_ulp(float(want.abs().max()))
    assert torch.equal(got3, got2)


@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("hd,gq", [(128, 4), (128, 7), (64, 4)])
def test_variant3_order_is_invisible(hd, gq, num_splits):
    c = _case(hd, gq, CTX_BATCHES[0])
    base = _run(c, 3, None, num_splits)
    assert not torch.isnan(base.float()).any()
    longest_first = ops.decode_order(c["lens"])
    for order in (longest_first, longest_first.flip(0).contiguous()):
        assert torch.equal(_run(c, 3, order, num_splits), base)


def test_variant3_leaves_out_alone_when_order_is_no_permutation():
    c = _case(128, 4, CTX_BATCHES[0])
    bad = torch.tensor([0, 7, -1], dtype=torch.int32, device="cuda")
    out = _run(c, 3, bad)
    assert torch.equal(out[0], _run(c, 3)[0])
    assert torch.isnan(out[1:].float()).all()


# contexts (17, 33, 100): smaller than every context, equal to one, larger
# than all of them
@pytest.mark.parametrize("window", [10, 33, 200])
@pytest.mark.parametrize("hd,gq", [(128, 4), (64, 2)])
def test_variant3_sliding_window(hd, gq, window):
    lens = (17, 33, 100)
    c = _case(hd, gq, lens)
    want = _want(hd, gq, lens, window=window)
    for num_splits in (1, 2):
        got = _run(c, 3, None, num_splits, window)
        torch.testing.assert_close(got.double().cpu(), want, **TOL)
        assert torch.equal(got, _run(c, 2, None, num_splits, window))


def test_variant3_split_kv():
    """S * KH = 6 workgroups: the dispatcher's own choice (num_splits = 0)
    is 32 splits, more than the 3 blocks of the short sequence."""
    lens = (300, 40, 257)
    c = _case(128, 4, lens)
    want = _want(128, 4, lens)
    split = _run(c, 3, None, 0)
    unsplit = _run(c, 3, None, 1)
    torch.testing.assert_close(split.double().cpu(), want, **TOL)
    torch.testing.assert_close(unsplit.double().cpu(), want, **TOL)
    # the two differ only in where the partial sums are merged
    torch.testing.assert_close(split.float(), unsplit.float(), **TOL)
    order = ops.decode_order(c["lens"])
    assert torch.equal(_run(c, 3, order, 0), split)
    assert torch.equal(split, _run(c, 2, None, 0))
    assert torch.equal(unsplit, _run(c, 2, None, 1))


def test_variant3_on_fp8_cache_runs_variant2():
    c = dict(_case(128, 4, CTX_BATCHES[0]))
    c["k"] = c["cpu"][1].to(torch.float8_e4m3fn).cuda()
    c["v"] = c["cpu"][2].to(torch.float8_e4m3fn).cuda()
    assert torch.equal(_run(c, 3), _run(c, 2))


@pytest.mark.parametrize("variant", [2, 3])
def test_out_argument_fills_one_buffer(variant):
    """A mixed step: prefill rows and decode rows written into one buffer
    equal the concatenation of the separate results, bit for bit."""
    hd, gq, lens = 128, 4, (17, 33, 100)
    c = _case(hd, gq, lens)
    qh = KH * gq
    g = torch.Generator().manual_seed(11)
    tp = 21  # a fresh 21-token prompt in blocks the decode batch leaves free
    q_pre = torch.randn((tp, qh, hd), generator=g).to(torch.bfloat16).cuda()
    used = set(c["bt"].cpu().flatten().tolist())
    free = [b for b in range(NB) if b not in used][:2]
    bt_pre = torch.tensor([free + [NB] * (MAX_BLOCKS - 2)],
                          dtype=torch.int32, device="cuda")
    rows = ops.prefill_tile_rows(qh, KH)
    tiles = torch.tensor(
        [[0, t0, t0, min(rows, tp - t0)] for t0 in range(0, tp, rows)],
        dtype=torch.int32, device="cuda")
    order = ops.decode_order(c["lens"])

    pre = ops.paged_attn_prefill_mfma(q_pre, c["k"], c["v"], bt_pre, tiles,
                                      c["scale"])
    dec = ops.paged_attn_decode(c["q"], c["k"], c["v"], c["bt"], c["lens"],
                                c["scale"], 0, order, variant=variant)
    assert torch.equal(dec, _run(c, variant, order, 0))

    S = len(lens)
    buf = torch.full((tp + S, qh, hd), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    r0 = ops.paged_attn_prefill_mfma(q_pre, c["k"], c["v"], bt_pre, tiles,
                                     c["scale"], out=buf[:tp])
    r1 = ops.paged_attn_decode(c["q"], c["k"], c["v"], c["bt"], c["lens"],
                               c["scale"], 0, order, out=buf[tp:],
                               variant=variant)
    assert r0.data_ptr() == buf.data_ptr()
    assert r1.data_ptr() == buf[tp:].data_ptr()
    assert not torch.isnan(buf.float()).any()
    assert torch.equal(buf, torch.cat([pre, dec], dim=0))


def test_out_argument_is_checked():
    c = _case(128, 4, CTX_BATCHES[0])
    wide = torch.empty((3, KH * 4, 256), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        ops.paged_attn_decode(c["q"], c["k"], c["v"], c["bt"], c["lens"],
                              c["scale"], out=wide[:, :, :128])
    with pytest.raises(ValueError):
        ops.paged_attn_decode(c["q"], c["k"], c["v"], c["bt"], c["lens"],
                              c["scale"], out=c["q"].float())
