"""int4 weight-only quantization on the CPU: config and CLI, the quantizer's
error bound, pack/unpack, the reference GEMM and a tiny-llama int4 engine.

Quantizer bound, per element, with s the stored (bf16) group scale and
Wd = bf16((q - z) * s):
    |w - Wd| <= 1.05 * s + 2^-8 * |Wd|.
Derivation, in steps of s: rounding w/s to an integer costs at most 0.5. The
codes cover [-z, 15 - z] steps. z = round(-lo/s) is within 0.5 of -lo/s, so
the window's low end is at most 0.5 above lo/s; the exact scale would put the
high end at hi/s, and rounding s to bf16 (relative 2^-9) moves the 15-step
span by at most 15 * 2^-9 ~ 0.03, so the clamp cuts at most ~0.53 beyond the
rounding's reach. Together below 1.05. The last term is the bf16 round of Wd
(2^-9 relative, doubled).
"""

import pytest
import torch
import torch.nn.functional as F

from production_stack_amd import ops
from production_stack_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)
from production_stack_amd.engine.engine import LLMEngine
from production_stack_amd.engine.models import llama
from production_stack_amd.engine.sampling import SamplingParams
from production_stack_amd.ops import reference

G = 128
PROMPT = list(range(20, 60))
PARAMS = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
PROJS = ("qkv_proj", "o_proj", "gate_up_proj", "down_proj")


def _config(**kw):
    return EngineConfig(
        model="tiny-llama",
        max_model_len=256,
        cache=CacheConfig(num_gpu_blocks=64, block_size=16),
        scheduler=SchedulerConfig(max_num_seqs=4, max_num_batched_tokens=256),
        **kw,
    )


def _first_logits(eng):
    """Generate from PROMPT; returns (tokens, logits of the first step)."""
    seen = []
    model = eng.runner.model
    real = model.compute_logits

    def shim(hidden):
        out = real(hidden)
        seen.append(out.detach().float().clone())
        return out

    model.compute_logits = shim
    try:
        toks = eng.generate([PROMPT], PARAMS)["offline-0"]
    finally:
        del model.compute_logits
    return toks, seen[0][-1]


# ------------------------------------------------------- config and CLI ----

def test_cli_accepts_int4():
    from production_stack_amd.engine.server import build_arg_parser

    ap = build_arg_parser()
    args = ap.parse_args(["tiny-llama", "--quantization", "int4"])
    assert args.quantization == "int4"
    assert ops.INT4_GROUP == G


def test_unknown_quantization_raises():
    with pytest.raises(ValueError):
        LLMEngine(_config(quantization="awq"), device="cpu")


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_other_quantizations_still_construct(quant):
    eng = LLMEngine(_config(quantization=quant), device="cpu")
    for layer in eng.runner.model.layers:
        assert getattr(layer, "int4_w", None) is None


# ------------------------------------------------------------ quantizer ----

def _weights():
    torch.manual_seed(0)
    w = torch.randn(256, 512) * 0.02
    w[3] = 0.0          # a row of zeros: the scale floor
    w[5, 130] = 1.0     # one outlier in group 1 of row 5
    w[9, :G] = w[9, :G].abs() + 0.01   # an all-positive group: z = 0
    w[11, :G] = -w[11, :G].abs() - 0.01  # an all-negative group: z = 15
    return w.bfloat16()


def test_quantizer_bound():
    w = _weights()
    packed, s, z = ops.int4_quantize_weight(w)
    N, K = w.shape
    assert packed.shape == (N, K // 2) and packed.dtype == torch.uint8
    assert s.shape == (N, K // G) and s.dtype == torch.bfloat16
    assert z.shape == (N, K // G) and z.dtype == torch.uint8
    q = ops.int4_unpack(packed)
    assert int(q.max()) <= 15 and int(z.max()) <= 15
    assert int(z[9, 0]) == 0 and int(z[11, 0]) == 15
    Wd = ops.int4_dequant(packed, s, z)
    assert Wd.dtype == torch.bfloat16 and Wd.shape == w.shape
    se = s.float().repeat_interleave(G, dim=1)
    ze = z.float().repeat_interleave(G, dim=1)
    assert torch.equal(Wd, ((q.float() - ze) * se).bfloat16())
    err = (w.double() - Wd.double()).abs()
    bound = 1.05 * se.double() + 2.0 ** -8 * Wd.double().abs()
    worst = float((err / bound).max())
    print(f"worst quantization error {worst:.3f} x bound")
    assert bool((err <= bound).all()), worst
    assert not bool(Wd[3].any()), "a zero row must dequantize to zeros"
    # the reference quantizer is what ops dispatches to
    rp, rs, rz = reference.int4_quantize_weight(w)
    assert torch.equal(rp, packed) and torch.equal(rs, s)
    assert torch.equal(rz, z)


def test_pack_unpack_round_trip():
    gen = torch.Generator().manual_seed(3)
    q = torch.randint(0, 16, (19, 384), dtype=torch.uint8, generator=gen)
    packed = ops.int4_pack(q)
    assert packed.shape == (19, 192) and packed.dtype == torch.uint8
    assert torch.equal(ops.int4_unpack(packed), q)
    # every nibble is used: distinct q give distinct packed rows
    q2 = q.clone()
    q2[7, 201] ^= 1
    assert int((ops.int4_pack(q2) != packed).sum()) == 1
    with pytest.raises(ValueError):
        ops.int4_pack(q[:, :192])


def test_reference_linear_is_linear_on_wd():
    w = _weights()
    packed, s, z = ops.int4_quantize_weight(w)
    torch.manual_seed(1)
    x = (torch.randn(7, 512) / 8).bfloat16()
    Wd = ops.int4_dequant(packed, s, z)
    want = F.linear(x.float(), Wd.float()).to(torch.bfloat16)
    assert torch.equal(reference.int4_linear(x, packed, s, z), want)
    assert torch.equal(ops.int4_linear(x, packed, s, z), want)


def test_supported_rule():
    assert ops.skinny_gemm_w4_supported(1, 64, 128)
    assert ops.skinny_gemm_w4_supported(256, 6144, 4096)
    for bad in [(0, 64, 128), (257, 64, 128), (16, 96, 128), (16, 64, 192),
                (16, 64, 64), (16, 32, 128)]:
        assert not ops.skinny_gemm_w4_supported(*bad), bad


# --------------------------------------------------------------- engine ----

@pytest.fixture(scope="module")
def engines():
    int4 = LLMEngine(_config(quantization="int4"), device="cpu")
    bf16 = LLMEngine(_config(), device="cpu")
    other = LLMEngine(_config(seed=1), device="cpu")
    return int4, bf16, other


def test_int4_engine_generates(engines):
    int4, _, _ = engines
    for layer in int4.runner.model.layers:
        assert set(layer.int4_w) == {"qkv", "o", "gate_up", "down"}
        for pname in PROJS:
            assert getattr(layer, pname).numel() == 0, pname
        for packed, s, z in layer.int4_w.values():
            assert packed.dtype == torch.uint8
            assert s.dtype == torch.bfloat16 and z.dtype == torch.uint8
            assert s.shape == z.shape == (packed.shape[0],
                                          packed.shape[1] * 2 // G)
    toks = int4.generate([PROMPT], PARAMS)["offline-0"]
    assert len(toks) == 8


def test_int4_logits_close_to_bf16(engines):
    """Sanity ordering, not a tolerance: the int4 engine's first-step logits
    are nearer to the bf16 engine's (same seed) than a different-seed bf16
    engine's are."""
    int4, bf16, other = engines
    _, l4 = _first_logits(int4)
    _, lb = _first_logits(bf16)
    _, lo = _first_logits(other)
    d_quant = float((l4 - lb).norm())
    d_seed = float((lo - lb).norm())
    print(f"|int4 - bf16| = {d_quant:.4f}, |other seed - bf16| = {d_seed:.4f}")
    assert d_quant < d_seed


def test_unshardable_projection_stays_bf16(caplog):
    """A projection whose local shape the int4 GEMM does not take stays
    bf16, and one log line says so."""
    import logging

    eng = LLMEngine(_config(), device="cpu")
    model = eng.runner.model
    layer = model.layers[0]
    layer.o_proj.data = layer.o_proj.data[:96].contiguous()  # N % 64 != 0
    with caplog.at_level(logging.WARNING):
        model.quantize_int4()
    assert set(layer.int4_w) == {"qkv", "gate_up", "down"}
    assert layer.o_proj.shape == (96, 128)
    assert set(model.layers[1].int4_w) == {"qkv", "o", "gate_up", "down"}
    lines = [r for r in caplog.records if "o_proj" in r.getMessage()]
    assert len(lines) == 1


def test_bf16_forward_never_calls_int4(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("int4_linear called without quantization")

    monkeypatch.setattr(ops, "int4_linear", boom)
    assert llama.ops is ops
    eng = LLMEngine(_config(), device="cpu")
    toks = eng.generate([PROMPT], PARAMS)["offline-0"]
    assert len(toks) == 8
