"""GPU tests of the chunked-prefill attention kernels at their tile, split,
page and window edges: paged_attn_prefill_mfma variant 5
(csrc/prefill_mfma32.hip) and variant 3 (csrc/prefill_mfma.hip), and the
VALU paged_attn_prefill (csrc/attention.hip).

Every case is one of tests/attention_criteria.py's CASES and is held to that
module's criterion: an fp64 reference, one bf16 rounding, and twice the
per-row deviation of a model that makes the kernel's own intermediate
roundings. tests/test_attention_criteria_cpu.py shows on the same cases that
this bound rejects off-by-one masks, a dropped key, swapped pages, a wrong
kv head, a skipped rescale and a split left out of the merge.

Block tables are shuffled; table padding points at a NaN block; the unwritten
tail of every last page is loud; `out` starts as NaN; every call forces its
variant.

Worst error over bound measured on an MI355X, at F = 2:

    kernel      bf16 KV   fp8 KV
    variant 5   0.986     0.916
    variant 3   0.984     0.914
    VALU        0.990     -

Variant 5 ran 1, 2, 3, 5, 6 and 8 splits. The first model (P rounded against
the row's true maximum) put variant 5 at 2.43x on v5_peaked_gq4_s1: defer-max
(csrc/prefill_mfma32.hip, `grew` / PS_RESCALE_THR32, and the bf16 rounding of
P in `p4[j] = ps_f32_to_bf16(...)`) rounds a dominant P that is not 1 against
a lagging maximum, while the row sum keeps it unrounded. The model now walks
the 64-key chunks with the kernels' own rescale rule; no kernel changed.
"""

import functools

import pytest
import torch

from production_stack_amd import ops
from tests import attention_criteria as ac
from tests.elementwise_criteria import assert_bits_equal

pytestmark = pytest.mark.gpu

NAN = float("nan")


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _names(kernel):
    return sorted(n for n, s in ac.CASES.items() if s.kernel == kernel)


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The case's inputs on the GPU, uploaded once and never modified."""
    c = ac.case(name)
    return dict(q=c.q.cuda(), k=c.k.cuda(), v=c.v.cuda(), bt=c.bt.cuda(),
                tiles=c.tiles.cuda(), token_seq=c.token_seq.cuda(),
                token_pos=c.token_pos.cuda())


def _mfma(name, variant, q=None, out=None):
    s, c, d = ac.CASES[name], ac.case(name), _dev(name)
    q = d["q"] if q is None else q
    if out is None:
        out = torch.full(c.q.shape, NAN, dtype=torch.bfloat16, device="cuda")
    res = ops.paged_attn_prefill_mfma(q, d["k"], d["v"], d["bt"], d["tiles"],
                                      c.scale, s.window, variant, out=out)
    assert res.data_ptr() == out.data_ptr()
    return res


def _valu(name, q=None, out=None):
    from production_stack_amd import _C

    s, c, d = ac.CASES[name], ac.case(name), _dev(name)
    q = d["q"] if q is None else q
    if out is None:
        out = torch.full(c.q.shape, NAN, dtype=torch.bfloat16, device="cuda")
    _C.paged_attn_prefill(out, q, d["k"], d["v"], d["bt"], d["token_seq"],
                          d["token_pos"], c.scale, s.window)
    return out


def _check(name, got, kernel):
    worst = ac.check(got, ac.case_yardstick(name), f"{kernel} {name}")
    print(f"WORST {kernel} {'fp8' if ac.CASES[name].fp8 else 'bf16'} "
          f"{name} {worst:.3f}")


# ---------------------------------------------------------------------------
# variant 5
# ---------------------------------------------------------------------------
def test_split_rule_is_the_extensions():
    from production_stack_amd import _C

    for nt in (1, 2, 7, 8, 12, 18, 35, 36, 125, 249, 250, 251):
        for gq in (1, 2, 3, 4, 6, 7, 8):
            assert _C.prefill_mfma32_splits(nt, ac.KH, gq) == \
                ac.v5_splits(nt, ac.KH, gq), (nt, gq)


@pytest.mark.parametrize("name", _names("v5"))
def test_variant5(name):
    from production_stack_amd import _C

    s, c = ac.CASES[name], ac.case(name)
    assert ops.prefill_tile_rows(c.qh, ac.KH) == s.tile_rows \
        or ops.PREFILL_VARIANT != 5
    splits = _C.prefill_mfma32_splits(c.tiles.shape[0], ac.KH, s.gq)
    if s.splits is not None:
        assert splits == s.splits, (name, splits)
    print(f"{name}: {splits} splits, {c.tiles.shape[0]} tiles of up to "
          f"{s.tile_rows} rows")
    _check(name, _mfma(name, 5), "v5")


@pytest.mark.parametrize("want", [1, 2, 3, 5, 8])
def test_variant5_split_counts_on_purpose(want):
    from production_stack_amd import _C

    name = f"v5_splits{want}"
    c = ac.case(name)
    assert _C.prefill_mfma32_splits(c.tiles.shape[0], ac.KH,
                                    ac.CASES[name].gq) == want
    if want == 8:
        # a context of 64 or fewer leaves splits 1..7 without a chunk; rows
        # 100..127 have no visible key in the chunk that begins at token 128
        assert min(c.seq_len) <= 64
        assert (0, 100, 50) in c.chunks


# ---------------------------------------------------------------------------
# variant 3 and the VALU kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("v3"))
def test_variant3(name):
    _check(name, _mfma(name, 3), "v3")


@pytest.mark.parametrize("name", _names("valu"))
def test_valu(name):
    _check(name, _valu(name), "valu")


# ---------------------------------------------------------------------------
# layout: q a column slice of the packed qkv buffer, out a row slice
# ---------------------------------------------------------------------------
def _qkv_slice(name):
    c = ac.case(name)
    T, QH, hd = c.q.shape
    buf = torch.full((T, (QH + 2 * ac.KH) * hd), NAN, dtype=torch.bfloat16,
                     device="cuda")
    buf[:, :QH * hd] = _dev(name)["q"].reshape(T, QH * hd)
    q = buf[:, :QH * hd].unflatten(1, (QH, hd))
    assert q.stride() == ((QH + 2 * ac.KH) * hd, hd, 1)
    return q


def _out_slice(name):
    T, QH, hd = ac.case(name).q.shape
    big = torch.full((T + 7, QH, hd), NAN, dtype=torch.bfloat16,
                     device="cuda")
    return big, big[3:3 + T]


@pytest.mark.parametrize("name,variant", [
    ("v5_gq4_bf16", 5), ("v5_gq1_fp8", 5), ("v5_splits1", 5),
    ("v3_gq7_bf16", 3), ("valu_hd64_gq2_w0", 0), ("valu_hd128_gq4_w17", 0)])
def test_strided_q_and_sliced_out(name, variant):
    run = _valu if variant == 0 else \
        functools.partial(_mfma, variant=variant)
    plain = run(name)
    big, out = _out_slice(name)
    before = big.clone()
    got = run(name, q=_qkv_slice(name), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_bits_equal(got, plain, name + " strided q / sliced out")
    assert_bits_equal(big[:3], before[:3], name + " rows before the slice")
    assert_bits_equal(big[3 + got.shape[0]:], before[3 + got.shape[0]:],
                      name + " rows after the slice")
    _check(name, got, {5: "v5", 3: "v3", 0: "valu"}[variant])


# ---------------------------------------------------------------------------
# host checks of the two bindings: each bad call must raise before a launch
# ---------------------------------------------------------------------------
def _args(name="v5_splits8"):
    c, d = ac.case(name), _dev(name)
    out = torch.full(c.q.shape, NAN, dtype=torch.bfloat16, device="cuda")
    return dict(out=out, q=d["q"], k_cache=d["k"], v_cache=d["v"],
                block_tables=d["bt"], tile_info=d["tiles"], scale=c.scale,
                variant=5, window=0)


def _valu_args(name="valu_hd64_gq2_w0"):
    c, d = ac.case(name), _dev(name)
    out = torch.full(c.q.shape, NAN, dtype=torch.bfloat16, device="cuda")
    return [out, d["q"], d["k"], d["v"], d["bt"], d["token_seq"],
            d["token_pos"], c.scale, 0]


def _raises_mfma(**bad):
    from production_stack_amd import _C

    a = _args()
    a.update(bad)
    with pytest.raises(RuntimeError):
        _C.paged_attn_prefill_mfma(**a)
    # the refused call wrote nothing
    assert torch.isnan(a["out"].float()).all() or "out" in bad


def _raises_valu(i, bad):
    from production_stack_amd import _C

    a = _valu_args()
    a[i] = bad
    with pytest.raises(RuntimeError):
        _C.paged_attn_prefill(*a)


def test_mfma_checks_q():
    q = _args()["q"]
    _raises_mfma(q=q.half())
    _raises_mfma(q=q.cpu())
    _raises_mfma(q=q.reshape(q.shape[0], -1))
    _raises_mfma(q=q[:, :, :64])                      # stride(1) != hd
    _raises_mfma(q=q.transpose(1, 2).contiguous().transpose(1, 2))


def test_mfma_checks_out_shape():
    q = _args()["q"]
    T, QH, hd = q.shape
    for shape in ((T + 1, QH, hd), (T, QH * hd), (T, QH // 2, hd)):
        _raises_mfma(out=torch.empty(shape, dtype=torch.bfloat16,
                                     device="cuda"))


def test_mfma_checks_tile_info_shape():
    tiles = _args()["tile_info"]
    _raises_mfma(tile_info=tiles.reshape(-1))
    _raises_mfma(tile_info=tiles[:, :3].contiguous())


def test_mfma_checks_block_tables_rank():
    _raises_mfma(block_tables=_args()["block_tables"].reshape(-1))


def test_mfma_checks_caches_agree():
    a = _args()
    k, v = a["k_cache"], a["v_cache"]
    _raises_mfma(v_cache=v[:-1].contiguous())
    _raises_mfma(v_cache=v.to(torch.float8_e4m3fn))
    _raises_mfma(k_cache=k[..., :64].contiguous(),
                 v_cache=v[..., :64].contiguous())     # size(3) != hd


def test_mfma_checks_window():
    _raises_mfma(window=-1)


@pytest.mark.parametrize("variant", [0, 2, 6, -1])
def test_mfma_checks_variant(variant):
    _raises_mfma(variant=variant)


def test_mfma_without_tiles_launches_nothing():
    from production_stack_amd import _C

    a = _args()
    a["tile_info"] = torch.empty((0, 4), dtype=torch.int32, device="cuda")
    for variant in (3, 5):
        a["variant"] = variant
        _C.paged_attn_prefill_mfma(**a)
        assert torch.isnan(a["out"].float()).all()


def test_valu_checks_q():
    q = _valu_args()[1]
    _raises_valu(1, q.half())
    _raises_valu(1, q.cpu())
    _raises_valu(1, q.reshape(q.shape[0], -1))
    _raises_valu(1, q[:, :, :32])


def test_valu_checks_out_shape():
    q = _valu_args()[1]
    T, QH, hd = q.shape
    _raises_valu(0, torch.empty((T + 1, QH, hd), dtype=torch.bfloat16,
                                device="cuda"))


def test_valu_checks_block_tables_rank():
    _raises_valu(4, _valu_args()[4].reshape(-1))


def test_valu_checks_caches_agree():
    v = _valu_args()[3]
    _raises_valu(3, v[:-1].contiguous())
    _raises_valu(3, v[..., :32].contiguous())


def test_valu_checks_window():
    _raises_valu(8, -1)


def test_valu_checks_token_arrays():
    _raises_valu(5, _valu_args()[5][:-1].contiguous())


def test_valu_without_rows_launches_nothing():
    from production_stack_amd import _C

    a = _valu_args()
    e = torch.empty((0,), dtype=torch.int32, device="cuda")
    _C.paged_attn_prefill(a[0][:0], a[1][:0], a[2], a[3], a[4], e, e,
                          a[7], 0)
    assert torch.isnan(a[0].float()).all()
