"""paged_attn_prefill_mfma variant 5 at head_dim 64 (csrc/prefill_mfma64.hip),
bf16 and fp8 KV, held to tests/attention_criteria.py's criterion at its own
F = 2: an fp64 reference, one bf16 rounding, and twice the per-row deviation of
the "mfma" rounding model (wave_rows = 32, the split count the call runs).

Inputs as in tests/test_prefill_edges_gpu.py: shuffled block tables, table
padding at a NaN block, loud page tails, `out` NaN-filled.

Worst error over bound measured on an MI355X, at F = 2 (1, 3 and 8 splits
ran):

    bf16 KV   0.983  (peaked)
    fp8 KV    0.941  (edge_gq4_fp8)
"""

import functools

import pytest
import torch

from production_stack_amd import ops
from tests import attention_criteria as ac
from tests.elementwise_criteria import assert_bits_equal

pytestmark = pytest.mark.gpu

HD = 64
EDGE = "edge"  # chunks that depend on the tile rows of the case's gq

# (id, gq, chunks, peaked, fp8, window, splits the case must run or None)
TABLE = [(f"edge_gq{gq}_bf16", gq, EDGE, False, False, 0, None)
         for gq in (1, 2, 4, 8)]
TABLE += [(f"edge_gq{gq}_fp8", gq, EDGE, False, True, 0, None)
          for gq in (1, 4)]
TABLE += [
    ("splits1", 7, ac.scattered_chunks(36), False, False, 0, 1),
    ("splits3", 7, ac.scattered_chunks(12), False, False, 0, 3),
    ("splits8", 4, ac.TWO_TILES, False, False, 0, 8),
    ("peaked", 4, ac.FOUR_TILES, True, False, 0, 8),
]
TABLE += [(f"w{w}_bf16", 4, ac.WINDOW_OWN, False, False, w, None)
          for w in (1, 63, 64, 65)]
TABLE += [("w65_fp8", 4, ac.WINDOW_OWN, False, True, 65, None)]


@functools.lru_cache(maxsize=None)
def _case(gq, chunks, peaked, fp8):
    """Inputs built once, uploaded once and never modified."""
    rows = ac.v5_tile_rows(gq)
    if chunks == EDGE:
        chunks = ac.edge_chunks(rows)
    seed = 64 + 31 * gq + 17 * peaked + 3 * fp8 + len(chunks)
    c = ac.build_case(seed, HD, gq, chunks, rows, peaked, fp8)
    dev = {n: getattr(c, n).cuda() for n in ("q", "k", "v", "bt", "tiles")}
    return c, dev


def _run(c, d, window, q=None):
    out = torch.full(c.q.shape, float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    return ops.paged_attn_prefill_mfma(d["q"] if q is None else q, d["k"],
                                       d["v"], d["bt"], d["tiles"], c.scale,
                                       window, variant=5, out=out)


@pytest.mark.parametrize("name,gq,chunks,peaked,fp8,window,splits", TABLE,
                         ids=[t[0] for t in TABLE])
def test_hd64(name, gq, chunks, peaked, fp8, window, splits):
    c, d = _case(gq, chunks, peaked, fp8)
    assert ops.prefill_mfma_supported(HD)
    n_splits = ac.v5_splits(c.tiles.shape[0], ac.KH, gq)
    assert splits is None or n_splits == splits
    ys = ac.yardstick(c, window, "mfma", wave_rows=32, n_splits=n_splits)
    worst = ac.check(_run(c, d, window), ys, name)
    print(f"WORST hd64 {'fp8' if fp8 else 'bf16'} {name} {n_splits} splits "
          f"{worst:.3f}")


def test_hd64_strided_q():
    """q as a row slice of the packed qkv buffer: bit-identical."""
    c, d = _case(4, EDGE, False, False)
    T, QH, hd = c.q.shape
    buf = torch.full((T, (QH + 2 * ac.KH) * hd), float("nan"),
                     dtype=torch.bfloat16, device="cuda")
    buf[:, :QH * hd] = d["q"].reshape(T, QH * hd)
    q = buf[:, :QH * hd].unflatten(1, (QH, hd))
    assert q.stride() == ((QH + 2 * ac.KH) * hd, hd, 1)
    assert_bits_equal(_run(c, d, 0, q=q), _run(c, d, 0), "strided q")
