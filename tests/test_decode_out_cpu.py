"""ops.paged_attn_decode(out=...) on CPU tensors: same result as without."""

import pytest
import torch

from production_stack_amd import ops


def _problem():
    g = torch.Generator().manual_seed(4)
    k = torch.randn((9, 2, 16, 64), generator=g).to(torch.bfloat16)
    v = torch.randn((9, 2, 16, 64), generator=g).to(torch.bfloat16)
    q = torch.randn((3, 4, 64), generator=g).to(torch.bfloat16)
    bt = torch.tensor([[5, 0, 0], [2, 7, 1], [8, 3, 0]], dtype=torch.int32)
    lens = torch.tensor([1, 33, 17], dtype=torch.int32)
    return q, k, v, bt, lens, 0.125


@pytest.mark.parametrize("window", [0, 10])
def test_out_matches_no_out_on_cpu(window):
    args = _problem()
    want = ops.paged_attn_decode(*args, window)
    buf = torch.full((5, 4, 64), float("nan"), dtype=torch.bfloat16)
    got = ops.paged_attn_decode(*args, window, out=buf[2:])
    assert got.data_ptr() == buf[2:].data_ptr()
    assert torch.equal(buf[2:], want)
    assert torch.isnan(buf[:2].float()).all()


def test_out_is_checked_on_cpu():
    args = _problem()
    with pytest.raises(ValueError):
        ops.paged_attn_decode(*args, out=torch.empty((3, 4, 32)))
    with pytest.raises(ValueError):
        ops.paged_attn_decode(
            *args, out=torch.empty((3, 4, 128),
                                   dtype=torch.bfloat16)[:, :, :64])
