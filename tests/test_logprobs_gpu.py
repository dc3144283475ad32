"""ops.logprobs (csrc/logprobs.hip) against its contract in float64.

Ids must match exactly: equal logits are ordered by ascending token id, so
they are a function of the row. Values are within 1e-4 absolute: bf16 inputs
are exact, the fp32 exponent argument (magnitude <= ~100) costs <= ~6e-6
relative per term, exp2 ~1 ulp, the 2^-40 truncation <= 1.4e-7 of Z >= 1 and
the final subtraction at magnitude <= 64 <= 4e-6: about 1e-5, a 10x margin.
"""

import pytest
import torch

from production_stack_amd import ops

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def contract(logits, token_ids, n):
    """(lp, top_ids, top_lp) of every row in float64, on the CPU."""
    x = logits.cpu().double()
    nan = x.isnan()
    lp_all = torch.log_softmax(x.masked_fill(nan, NEG_INF), dim=-1)
    lp = lp_all.gather(1, token_ids.cpu().unsqueeze(1)).squeeze(1)
    R, V = x.shape
    # stable sort on (-x, id); -inf gets a finite key so NaN alone is last
    order = torch.sort(x.clamp(min=-1e300).masked_fill(nan, NEG_INF), dim=-1,
                       descending=True, stable=True).indices[:, :n]
    ids = torch.full((R, n), -1, dtype=torch.int32)
    vals = torch.full((R, n), NEG_INF, dtype=torch.float64)
    ids[:, : min(n, V)] = order.int()
    vals[:, : min(n, V)] = lp_all.gather(1, order)
    return lp, ids, vals


def check(logits, token_ids, n, rows=None):
    lp, ids, vals = ops.logprobs(logits.cuda(), token_ids.cuda(), n,
                                 None if rows is None else rows.cuda())
    want = contract(logits, token_ids, n)
    if rows is not None:
        want = tuple(w[rows.long()] for w in want)
    assert ids.dtype == torch.int32 and ids.shape == want[1].shape
    assert torch.equal(ids.cpu(), want[1])
    torch.testing.assert_close(lp.cpu().double(), want[0], atol=1e-4, rtol=0)
    torch.testing.assert_close(vals.cpu().double(), want[2], atol=1e-4,
                               rtol=0)
    return lp, ids, vals


@pytest.mark.parametrize("n", [0, 1, 5, 20])
@pytest.mark.parametrize("V", [8, 1000, 1001, 4104, 152064])
def test_random_rows(V, n):
    g = torch.Generator().manual_seed(V + n)
    logits = (torch.randn(3, V, generator=g) * 4).bfloat16()
    check(logits, torch.randint(0, V, (3,), generator=g), n)


@pytest.mark.parametrize("n", [1, 5, 20])
@pytest.mark.parametrize("all_ties", [False, True])
def test_threshold_ties_across_lanes_chunks_and_waves(n, all_ties):
    """Three distinct values. The tie class of the threshold sits at ids 5, 6
    (one lane) and every 997th id after (chunks and waves apart); with n - 1
    larger values exactly one tie is taken, with none exactly n."""
    V = 20000
    row = torch.full((V,), -1.5)
    ties = sorted({6, *range(5, V, 997)})
    assert len(ties) > 20
    row[ties] = 0.75
    if not all_ties:
        row[torch.arange(n - 1) * 1013 + 2] = 3.0
    flat = torch.full((V,), 0.75)  # every logit equal: ids 0 .. n - 1
    logits = torch.stack([row, flat]).bfloat16()
    _, ids, _ = check(logits, torch.tensor([5, V - 1]), n)
    assert ids[1].tolist() == list(range(n))


def test_neg_inf_and_nan():
    V = 20000
    row = torch.full((V,), NEG_INF)
    row[[40, 7000, 19999]] = torch.tensor([1.0, 2.0, 1.0])
    row[1] = float("nan")
    _, ids, vals = check(row.bfloat16().unsqueeze(0).repeat(2, 1),
                         torch.tensor([1, 40]), 5)
    assert ids[0].tolist() == [7000, 40, 19999, 0, 2]  # the NaN at 1 is last
    assert vals[0, 3:].tolist() == [NEG_INF, NEG_INF]


def test_rows_and_batch_independence():
    V = 4104
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(5, V, generator=g) * 4).bfloat16()
    token_ids = torch.tensor([7, 0, 100, 9, V - 1])
    rows = torch.tensor([4, 1], dtype=torch.int32)
    got = check(logits, token_ids, 5, rows)
    for m, r in enumerate(rows.tolist()):
        alone = ops.logprobs(logits[r:r + 1].clone().cuda(),
                             token_ids[r:r + 1].cuda(), 5)
        for a, b in zip(alone, got):
            assert torch.equal(a[0], b[m])


def test_host_checks():
    logits = torch.zeros(2, 64, dtype=torch.bfloat16, device="cuda")
    tok = torch.zeros(2, dtype=torch.long, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        ops.logprobs(logits, tok, 21)
    with pytest.raises((ValueError, RuntimeError)):
        ops.logprobs(logits.float(), tok, 1)
    with pytest.raises((ValueError, RuntimeError)):
        ops.logprobs(logits, tok, 1, torch.zeros(1, dtype=torch.long,
                                                 device="cuda"))
