"""The prefill-attention criterion of tests/attention_criteria.py accepts
honest evaluations and rejects subtly wrong kernels, on every case that
tests/test_prefill_edges_gpu.py runs on the GPU. No GPU is needed: the
mutants are CPU functions, and the seeds are fixed.

A mutant is rejected when at least one element is beyond the bound. In
cases whose contexts are all 256 or more, at least a quarter of the (row,
head) pairs the mutant touches must be, so that detection does not hang on
a single short row."""

import functools

import pytest
import torch

from production_stack_amd.ops import reference
from tests import attention_criteria as ac

NAMES = sorted(ac.CASES)


@functools.lru_cache(maxsize=None)
def _reference_fp32(name):
    """ops.reference.paged_attn_prefill in fp32 on the CPU, rounded to bf16.
    Window-free cases that share inputs share the result."""
    s = ac.CASES[name]
    c = ac.case(name)
    k, v = c.k, c.v
    if s.fp8:
        k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
    return reference.paged_attn_prefill(
        c.q, k, v, c.bt, c.token_seq, c.token_pos, c.scale, s.window)


def test_split_rule_matches_the_cases():
    """Every variant-5 case that names a split count gets it from the
    dispatcher's rule; the rule itself is asserted against the extension on
    the GPU."""
    seen = set()
    for name, s in ac.CASES.items():
        if s.kernel != "v5":
            continue
        n = ac.expected_splits(name)
        seen.add(n)
        if s.splits is not None:
            assert n == s.splits, (name, n)
    assert {1, 2, 3, 5, 8} <= seen, seen


def test_case_builder_poison_and_tables():
    c = ac.case("v5_gq4_bf16")
    nb = c.k.shape[0] - 1
    assert torch.isnan(c.k[nb].float()).all()
    assert torch.isnan(c.v[nb].float()).all()
    assert torch.isfinite(c.k[:nb].float()).all()
    live = []
    for s, n in enumerate(c.seq_len):
        pages = -(-n // ac.BS)
        live += c.bt[s, :pages].tolist()
        assert (c.bt[s, pages:] == nb).all() and c.bt.shape[1] > pages
        tail = n % ac.BS
        if tail:
            assert (c.v[int(c.bt[s, pages - 1]), :, tail:] == 1024).all()
    assert len(set(live)) == len(live) and nb not in live
    assert live != sorted(live), "tables must not be contiguous"
    # every row of q belongs to exactly one tile
    cover = torch.zeros(c.q.shape[0], dtype=torch.int32)
    for s, t0, p0, n in c.tiles.tolist():
        cover[t0:t0 + n] += 1
        assert (c.token_pos[t0:t0 + n] == torch.arange(p0, p0 + n)).all()
        assert (c.token_seq[t0:t0 + n] == s).all()
    assert (cover == 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_criterion_accepts_fp32_reference(name):
    ys = ac.case_yardstick(name)
    worst = ac.check(_reference_fp32(name), ys, name + " fp32 reference")
    print(f"{name}: fp32 reference at {worst:.3f} of the bound")


@pytest.mark.parametrize("name", NAMES)
def test_criterion_accepts_rounding_model(name):
    ys = ac.case_yardstick(name)
    worst = ac.check(ys.model.to(torch.float32).to(torch.bfloat16), ys,
                     name + " rounding model")
    print(f"{name}: rounding model at {worst:.3f} of the bound")


@pytest.mark.parametrize("name", NAMES)
def test_criterion_rejects_every_mutant(name):
    s = ac.CASES[name]
    c = ac.case(name)
    ys = ac.case_yardstick(name)
    splits = ac.expected_splits(name)
    muts = ac.mutants(c, s.window, s.model, s.peaked, splits, s.wave_rows)
    assert {"causal_lt", "causal_le_q_plus_1",
            "q_head_0_reads_kv_head_1"} <= set(muts)
    assert ("skip_last_rescale" in muts) == (s.peaked and s.model == "mfma")
    serving = ac.min_context(name) >= 256
    for mname, (kw, touched) in muts.items():
        assert touched.any(), (name, mname)
        got = ac.attend(c, s.window, s.model, **ac.model_kw(name), **kw)
        got = got.to(torch.float32).to(torch.bfloat16)
        rej = ac.rejected_pairs(got, ys)
        n_rej, n_touched = int((rej & touched).sum()), int(touched.sum())
        print(f"{name} {mname}: {n_rej}/{n_touched} touched pairs rejected")
        assert n_rej >= 1, (name, mname)
        if serving:
            assert 4 * n_rej >= n_touched, (name, mname, n_rej, n_touched)
