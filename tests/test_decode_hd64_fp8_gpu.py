"""paged_attn_decode with an fp8 e4m3 KV cache at head_dim 64: what
test_kernels_gpu.test_paged_attn_decode_fp8_kv checks at head_dim 128
(reference on the dequantized cache, 3e-2 abs/rel), for every GQA ratio the
head_dim-64 dispatcher knows and with and without split-KV."""

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.ops import reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("num_splits", [1, 4])
@pytest.mark.parametrize("gq", [1, 2, 4, 8])
def test_paged_attn_decode_fp8_kv_hd64(gq, num_splits):
    from production_stack_amd import _C

    assert ops.HAVE_EXT
    torch.manual_seed(9)
    kh, hd, bs = 2, 64, 16
    qh = kh * gq
    S = 3
    seq_lens = torch.tensor([5, 300, 64], dtype=torch.int32)
    max_blocks = 20
    nb = S * max_blocks + 1
    k8 = torch.randn((nb, kh, bs, hd), dtype=torch.bfloat16,
                     device="cuda").to(torch.float8_e4m3fn)
    v8 = torch.randn((nb, kh, bs, hd), dtype=torch.bfloat16,
                     device="cuda").to(torch.float8_e4m3fn)
    block_tables = torch.arange(
        1, S * max_blocks + 1, dtype=torch.int32).reshape(S, max_blocks)
    q = torch.randn((S, qh, hd), dtype=torch.bfloat16, device="cuda")
    want = reference.paged_attn_decode(
        q.cpu(), k8.cpu().to(torch.bfloat16), v8.cpu().to(torch.bfloat16),
        block_tables, seq_lens, 1.0 / hd ** 0.5)
    out = torch.full_like(q, float("nan"))
    _C.paged_attn_decode(out, q, k8, v8, block_tables.cuda(),
                         seq_lens.cuda(), 1.0 / hd ** 0.5, num_splits, 1)
    torch.testing.assert_close(out.float().cpu(), want.float(), atol=3e-2,
                               rtol=3e-2)
