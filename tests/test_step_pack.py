"""The C++ step-input packer (csrc/step_pack.h via _C.pack_step_inputs)
against ModelRunner.prepare() on the CPU: every section must be equal in
value, dtype and shape. No GPU needed; skipped without the extension."""

from types import SimpleNamespace

import pytest
import torch

from production_stack_amd import ops
from production_stack_amd.engine.config import ARCHITECTURES
from production_stack_amd.engine.model_runner import ModelRunner
from production_stack_amd.engine.sampling import SamplingParams
from production_stack_amd.engine.scheduler import ScheduledSeq, SchedulerOutput
from production_stack_amd.engine.sequence import Sequence

pytestmark = pytest.mark.skipif(
    not ops.HAVE_EXT, reason="production_stack_amd._C is not built"
)

BS = 16
CFG = ARCHITECTURES["mini-llama"]
TILE = ops.prefill_tile_rows(CFG.num_q_heads, CFG.num_kv_heads)
BM = SimpleNamespace(block_size=BS)
PARAMS = SamplingParams(max_tokens=8, temperature=0.0)


def make_runner() -> ModelRunner:
    """A runner with just the state prepare()/prepare_native() read."""
    r = ModelRunner.__new__(ModelRunner)
    r.device = torch.device("cpu")
    r.model_cfg = CFG
    r.lora_slots = None
    r.lora_registry = None
    r.pipeline = None
    r.tp_coord = None
    r.native_prepare = True
    r._stage = [None, None]
    r._stage_i = 0
    r._prev_rows = {}
    r._prev_tokens_dev = None
    return r


_next_block = [7]


def make_seq(rid, n_prompt, computed, outputs=(), extra_blocks=0):
    """Sequence with `computed` tokens done and a block table that covers
    all of its tokens (+ extra_blocks), blocks numbered out of order."""
    seq = Sequence(rid, [(3 * i + len(rid)) % 2000 + 1
                         for i in range(n_prompt)], PARAMS)
    seq.output_token_ids = list(outputs)
    seq.num_computed = computed
    n_blocks = (seq.num_tokens + BS - 1) // BS + extra_blocks
    seq.block_table = []
    for _ in range(n_blocks):
        _next_block[0] = (_next_block[0] * 37 + 11) % 4093
        seq.block_table.append(_next_block[0])
    return seq


def prefill(rid, n_prompt, computed, rows, **kw):
    return ScheduledSeq(make_seq(rid, n_prompt, computed, **kw), rows)


def decode(rid, n_prompt, outputs, **kw):
    seq = make_seq(rid, n_prompt, n_prompt + len(outputs) - 1,
                   outputs=outputs, **kw)
    return ScheduledSeq(seq, 1)


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.dtype == b.dtype, what
    assert a.shape == b.shape, what
    assert torch.equal(a, b), what


def check_against_prepare(scheduled, prev_rows=None, prev_tokens=None):
    out = SchedulerOutput(scheduled=list(scheduled))
    r = make_runner()
    r._prev_rows = dict(prev_rows or {})
    r._prev_tokens_dev = prev_tokens
    got = r.prepare_native(out, BM)
    assert got is not None
    tok_n, meta_n, seqs_n, rows_n, prev_n, n_ph = got
    tok_o, meta_o, seqs_o, rows_o = r.prepare(out, BM)
    same(tok_n, tok_o, "tokens")
    same(rows_n, rows_o, "sample_rows")
    assert [s.request_id for s in seqs_n] == [s.request_id for s in seqs_o]
    for name in ("positions", "slot_mapping", "prefill_token_seq",
                 "prefill_token_pos", "prefill_block_tables",
                 "decode_seq_lens", "decode_block_tables", "prefill_tiles",
                 "lora_idx", "mm_rows", "mm_embeds"):
        same(getattr(meta_n, name), getattr(meta_o, name), name)
    assert meta_n.num_prefill_tokens == meta_o.num_prefill_tokens
    assert meta_n.num_decode_seqs == meta_o.num_decode_seqs
    assert meta_n.lora_groups == meta_o.lora_groups == []
    # prev_row: -1 on real tokens, the previous row on placeholders
    expect = []
    for ss in out.scheduled:
        if not ss.is_decode:
            expect += [-1] * ss.num_tokens
    for ss in out.scheduled:
        if ss.is_decode:
            ph = ss.seq.token_ids()[ss.seq.num_computed] < 0
            expect.append(r._prev_rows[ss.seq.request_id] if ph else -1)
    assert prev_n.dtype == torch.int32
    assert prev_n.tolist() == expect
    assert n_ph == sum(1 for e in expect if e >= 0)
    return got


def test_prefill_only():
    check_against_prepare([
        prefill("a", 300, 0, 300),     # whole prompt: last row sampled
        prefill("bb", 500, 100, 200),  # middle chunk: not sampled
    ])


def test_decode_only():
    check_against_prepare([
        decode("a", 5, [11]),                       # table of length 1
        decode("bb", 40, [3, 4, 5]),
        decode("ccc", 333, [9] * 20, extra_blocks=3),
    ])


def test_mixed_with_unequal_tables():
    check_against_prepare([
        prefill("p0", 2 * TILE + 3, 0, 2 * TILE + 3),
        prefill("p1", 50, 16, 34, extra_blocks=2),
        decode("d0", 3, [5]),                       # table of length 1
        decode("d1", 1000, [1, 2, 3]),
        # a 1-row chunk inside a prompt: one row, takes the decode path
        ScheduledSeq(make_seq("p2", 64, 10), 1),
    ])


def test_one_prefill_of_one_row():
    # a 1-token chunk is a decode row to prepare(): same here
    check_against_prepare([ScheduledSeq(make_seq("a", 20, 19), 1)])
    check_against_prepare([ScheduledSeq(make_seq("a", 1, 0), 1)])


@pytest.mark.parametrize("rows", [2, TILE - 1, TILE, TILE + 1, 3 * TILE])
def test_tile_edges(rows):
    check_against_prepare([
        prefill("a", rows + 40, 7, rows),
        prefill("b", rows, 0, rows),
    ])


@pytest.mark.parametrize("end", [4 * BS, 4 * BS + 1, 4 * BS - 1])
def test_chunk_end_at_block_boundary(end):
    # the chunk's last position is end-1: the last token of a block, the
    # first of the next one, and one before the boundary
    check_against_prepare([prefill("a", 200, 10, end - 10)])
    check_against_prepare([prefill("a", end, 0, end)])


def test_prefill_last_row_sampled_or_not():
    got = check_against_prepare([
        prefill("a", 90, 30, 60),   # reaches the prompt's end: sampled
        prefill("b", 90, 30, 59),   # one short: not sampled
        decode("d", 12, [4]),
    ])
    assert got[3].tolist() == [59, 119]
    assert [s.request_id for s in got[2]] == ["a", "d"]


def test_decode_placeholders():
    prev_tokens = torch.arange(100, 110)
    got = check_against_prepare(
        [
            prefill("p", 70, 0, 70),
            decode("d0", 12, [4, -1]),
            decode("d1", 30, [8]),
            decode("d2", 17, [-1]),
        ],
        prev_rows={"d0": 6, "d1": 2, "d2": 0},
        prev_tokens=prev_tokens,
    )
    tok, prev_row = got[0], got[4]
    assert prev_row.tolist() == [-1] * 70 + [6, -1, 0]
    assert got[5] == 2
    ops.resolve_placeholders(tok, prev_row, prev_tokens)
    assert tok[70:].tolist() == [106, 8, 100]


def test_unresolvable_placeholders_are_reported():
    r = make_runner()
    r._prev_tokens_dev = torch.arange(4)
    # inside a prefill chunk (preempted, readmitted for recompute)
    seq = make_seq("a", 20, 0, outputs=[5, -1])
    out = SchedulerOutput(scheduled=[ScheduledSeq(seq, 22)])
    assert r.prepare_native(out, BM) is None
    # a decode row the previous step did not sample
    out = SchedulerOutput(scheduled=[decode("d", 9, [-1])])
    assert r.prepare_native(out, BM) is None
    r._prev_rows = {"d": 1}
    assert r.prepare_native(out, BM) is not None
    # no previous sampled tensor at all
    r._prev_tokens_dev = None
    assert r.prepare_native(out, BM) is None


def raw_args(scheduled):
    desc, toks, tabs = [], [], []
    for ss in scheduled:
        seq = ss.seq
        start = seq.num_computed
        toks += seq.token_ids()[start:start + ss.num_tokens]
        desc += [start, ss.num_tokens, int(ss.is_decode), 1, -1]
        tabs.append(seq.block_table)
    return desc, toks, tabs


def test_prefill_placeholder_writes_nothing():
    seq = make_seq("a", 20, 0, outputs=[5, -1])
    desc, toks, tabs = raw_args([ScheduledSeq(seq, 22)])
    buf = torch.full((4096,), 0xAB, dtype=torch.uint8)
    status, _ = ops.pack_step_inputs(buf, desc, toks, tabs, BS, TILE)
    assert status == ops.PACK_PREFILL_PLACEHOLDER
    assert bool((buf == 0xAB).all())


def test_buffer_one_byte_too_small():
    scheduled = [prefill("p", 150, 0, 150), decode("d", 40, [3])]
    desc, toks, tabs = raw_args(scheduled)
    status, lay = ops.pack_step_inputs(
        torch.empty(0, dtype=torch.uint8), desc, toks, tabs, BS, TILE
    )
    assert status == ops.PACK_TOO_SMALL
    need = lay["total_bytes"]
    assert need > 0 and need % 16 == 0
    backing = torch.full((need + 64,), 0xCD, dtype=torch.uint8)
    status, lay2 = ops.pack_step_inputs(
        backing[: need - 1], desc, toks, tabs, BS, TILE
    )
    assert status == ops.PACK_TOO_SMALL
    assert lay2["total_bytes"] == need
    assert bool((backing == 0xCD).all())  # nothing written, guards intact
    status, _ = ops.pack_step_inputs(
        backing[:need], desc, toks, tabs, BS, TILE
    )
    assert status == ops.PACK_OK
    assert bool((backing[need:] == 0xCD).all())
    for key, off in lay.items():
        if key.startswith("off_"):
            assert off % 16 == 0 and 0 < off <= need


def test_bad_input_is_rejected():
    # a position past the block table, and a decode before a prefill
    seq = make_seq("a", 40, 0)
    seq.block_table = seq.block_table[:1]
    desc, toks, tabs = raw_args([ScheduledSeq(seq, 40)])
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    status, _ = ops.pack_step_inputs(buf, desc, toks, tabs, BS, TILE)
    assert status == ops.PACK_BAD_INPUT
    desc, toks, tabs = raw_args([decode("d", 9, [1]),
                                 prefill("p", 30, 0, 30)])
    status, _ = ops.pack_step_inputs(buf, desc, toks, tabs, BS, TILE)
    assert status == ops.PACK_BAD_INPUT


def test_staging_grows_and_alternates():
    r = make_runner()
    small = SchedulerOutput(scheduled=[decode("d", 9, [1])])
    big = SchedulerOutput(scheduled=[prefill("p", 9000, 0, 9000)])
    a = r.prepare_native(small, BM)
    b = r.prepare_native(small, BM)
    assert a[0].data_ptr() != b[0].data_ptr()  # two arenas
    kept = a[0].clone()
    c = r.prepare_native(big, BM)               # outgrows the first arena
    assert c[0].numel() == 9000
    assert torch.equal(c[0], r.prepare(big, BM)[0])
    assert torch.equal(b[0], kept)              # the other arena is intact
