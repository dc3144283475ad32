"""The pass criteria of tests/elementwise_criteria.py, checked without a GPU:
each accepts an honest fp32 evaluation of its op (what a correct kernel
computes) and rejects a subtly wrong one. The GPU tests in
tests/test_elementwise_edges_gpu.py apply the same criteria to the kernels, so
the rejections here are the evidence that they would catch such a kernel."""

import pytest
import torch

from tests import elementwise_criteria as ec

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(T, D, seed):
    """x, w in bf16; row 0 tiny (eps matters), row 1 zero, row 2 large."""
    g = _gen(seed)
    x = torch.randn(T, D, generator=g).to(BF16)
    w = torch.randn(D, generator=g).to(BF16)
    x[0] = (x[0].float() * 1e-3).to(BF16)
    x[1] = 0
    x[2] = (x[2].float() * 3e4).to(BF16)
    return x, w


def _norm_f32(x, w, eps, residual=None):
    v = x.float()
    if residual is not None:
        v = v + residual.float()
    inv = torch.rsqrt((v * v).sum(-1, keepdim=True) / v.shape[-1] + eps)
    return v * inv * w.float()


# ---------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------
def test_half_ulp_bf16_is_half_the_spacing():
    v = torch.tensor([1.0, 1.99, 2.0, 0.75, 3e4, 1e-30, 0.0], dtype=torch.float64)
    got = ec.half_ulp_bf16(v)
    # spacing of bf16 at v, from the format itself
    b = v.to(BF16)
    up = (b.view(torch.int16) + 1).view(BF16).double() - b.double()
    assert torch.equal(got[:6] * 2, up[:6])
    assert got[6] == 2.0 ** -134


def test_half_step_e4m3_matches_the_code_grid():
    codes = torch.arange(0, 0x7F, dtype=torch.uint8).view(FP8).float().double()
    gaps = codes[1:] - codes[:-1]
    assert torch.equal(ec.half_step_e4m3(codes[:-1])[1:] * 2, gaps[1:])
    assert ec.half_step_e4m3(torch.tensor([0.0, 1e-5, 448.0, 500.0],
                                          dtype=torch.float64)).tolist() == [
        2.0 ** -10, 2.0 ** -10, 16.0, 16.0]


# ---------------------------------------------------------------------------
# bf16 norm / silu
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 4104, 32768])
def test_bf16_criterion_accepts_fp32_norm_rejects_missing_eps(D):
    x, w = _rows(4, D, seed=D)
    ref = ec.ref_rms_norm(x, w, EPS)
    ec.assert_bf16_rounded(_norm_f32(x, w, EPS).to(BF16), ref, 0.0, "fp32")
    with pytest.raises(AssertionError):
        ec.assert_bf16_rounded(_norm_f32(x, w, 0.0).to(BF16), ref, 0.0, "no eps")
    # the old atol=rtol=2e-2 would not see a kernel that rounds twice
    twice = _norm_f32(x, w, EPS).to(BF16).float() * 1.002
    with pytest.raises(AssertionError):
        ec.assert_bf16_rounded(twice.to(BF16), ref, 0.0, "scaled 0.2%")


def test_bf16_criterion_fused_add_norms_the_unrounded_sum():
    x, w = _rows(4, 4096, seed=3)
    res = torch.randn(4, 4096, generator=_gen(4)).to(BF16)
    ref = ec.ref_rms_norm(x, w, EPS, residual=res)
    ec.assert_bf16_rounded(_norm_f32(x, w, EPS, res).to(BF16), ref, 0.0)
    assert ec.residual_sum_bf16(x, res).dtype == BF16


def test_bf16_criterion_accepts_fp32_silu():
    g = _gen(5)
    x = torch.randn(5, 2 * 1000, generator=g).to(BF16)
    x[0, :4] = torch.tensor([30.0, -30.0, 80.0, -80.0]).to(BF16)
    v = x.float()
    got = v[:, :1000] / (1 + torch.exp(-v[:, :1000])) * v[:, 1000:]
    ref = ec.ref_silu_and_mul(x)
    ec.assert_bf16_rounded(got.to(BF16), ref, 0.0)
    # sigmoid approximated by a clamp at -20 zeroes the far negative side
    wrong = torch.where(v[:, :1000] < -20, torch.zeros_like(got), got)
    with pytest.raises(AssertionError):
        ec.assert_bf16_rounded(wrong.to(BF16), ref, 0.0)


# ---------------------------------------------------------------------------
# fp8
# ---------------------------------------------------------------------------
def _fp8_quant_f32(vals, divisor=448.0):
    amax = vals.abs().amax(dim=1).clamp(min=1e-6)
    scale = amax / divisor
    return (vals * (1.0 / scale)[:, None]), scale


def _truncate_e4m3(r):
    """Round toward zero onto the e4m3 grid."""
    r64 = r.double()
    step = ec.half_step_e4m3(r64) * 2
    return (torch.sign(r64) * torch.floor(r64.abs() / step) * step).float()


@pytest.mark.parametrize("D", [8, 4096, 5120, 16384])
def test_fp8_criterion_accepts_fp32_rejects_wrong_casts(D):
    x, w = _rows(4, D, seed=100 + D)
    ref = ec.ref_rms_norm(x, w, EPS)
    vals = _norm_f32(x, w, EPS)
    r, scale = _fp8_quant_f32(vals)
    worst = ec.assert_fp8_rounded(r.to(FP8), scale, ref, "fp32")
    assert worst <= 1.0001
    assert scale[1] == pytest.approx(1e-6 / 448, rel=1e-6)  # the zero row
    with pytest.raises(AssertionError):
        ec.assert_fp8_rounded(_truncate_e4m3(r).to(FP8), scale, ref, "trunc")
    r240, s240 = _fp8_quant_f32(vals, divisor=240.0)
    with pytest.raises(AssertionError):
        ec.assert_fp8_rounded(r240.to(FP8), s240, ref, "amax/240")
    # small elements flushed to zero: inside the old 2*scale allowance
    flushed = torch.where(r.abs() < 1.0, torch.zeros_like(r), r)
    if D > 8:
        with pytest.raises(AssertionError):
            ec.assert_fp8_rounded(flushed.to(FP8), scale, ref, "flush")


def test_fp8_criterion_unit_scale():
    x = torch.randn(6, 64, generator=_gen(7)).to(BF16)
    ec.assert_fp8_rounded(x.to(FP8), None, x.double(), "cast")
    with pytest.raises(AssertionError):
        ec.assert_fp8_rounded(_truncate_e4m3(x.float()).to(FP8), None,
                              x.double(), "trunc")


# ---------------------------------------------------------------------------
# int8
# ---------------------------------------------------------------------------
def _kv_quant_f32(x, half_away=False):
    v = x.float()
    amax = v.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    f = (v * (1.0 / scale)[:, None]).clamp(-127, 127)
    if half_away:
        q = torch.sign(f) * torch.floor(f.abs() + 0.5)
    else:
        q = torch.round(f)
    return q.to(torch.int8), scale


@pytest.mark.parametrize("hd", [8, 64, 1024])
def test_int8_criterion_accepts_half_even_rejects_half_away(hd):
    x = ec.kv_rows(203, hd, seed=hd)
    q, s = _kv_quant_f32(x)
    ec.assert_int8_codes(q, s, x, "half-even")
    assert s[1] == 1.0 and int(q[1].abs().max()) == 0
    assert s[3] == 2.0 ** -5
    qa, sa = _kv_quant_f32(x, half_away=True)
    assert (qa != q).any()
    with pytest.raises(AssertionError):
        ec.assert_int8_codes(qa, sa, x, "half-away")
    off = q.clone()
    off[5, hd - 1] += 1 if off[5, hd - 1] < 127 else -1
    with pytest.raises(AssertionError):
        ec.assert_int8_codes(off, s, x, "one code off by one")
    with pytest.raises(AssertionError):
        ec.assert_int8_codes(q, s * (1 + 1e-5), x, "scale")


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
def _rope_f32(pos, heads, cos_sin, hd, rotate_all=False):
    T = heads.shape[0]
    v = heads.float().reshape(T, -1, hd).clone()
    cs = cos_sin[pos.long()]
    rot = cs.shape[1]
    c, s = cs[:, None, : rot // 2], cs[:, None, rot // 2 :]
    if rotate_all:  # treat the whole head as rotary, reusing the angles
        c = c.repeat(1, 1, hd // rot)
        s = s.repeat(1, 1, hd // rot)
        rot = hd
    half = rot // 2
    x1, x2 = v[..., :half].clone(), v[..., half:rot].clone()
    v[..., :half] = x1 * c - x2 * s
    v[..., half:rot] = x2 * c + x1 * s
    return v.reshape(T, -1).to(BF16)


@pytest.mark.parametrize("hd,rot", [(128, 128), (128, 64), (64, 32)])
def test_rope_criterion_accepts_fp32_rejects_full_rotation(hd, rot):
    g = _gen(hd + rot)
    T, H, max_pos = 5, 6, 97
    heads = torch.randn(T, H * hd, generator=g).to(BF16)
    pos = torch.tensor([0, max_pos - 1, 13, 50, 1], dtype=torch.int32)
    cs = ec.rope_table(max_pos, rot)
    ec.check_rope(_rope_f32(pos, heads, cs, hd), heads, pos, cs, hd, "fp32")
    if rot < hd:
        with pytest.raises(AssertionError):
            ec.check_rope(_rope_f32(pos, heads, cs, hd, rotate_all=True),
                          heads, pos, cs, hd, "rotates all of hd")
    # interleaved (GPT-J) pairing instead of neox halves
    v = heads.float().reshape(T, H, hd).clone()
    c = cs[pos.long()][:, None, : rot // 2]
    s = cs[pos.long()][:, None, rot // 2 :]
    x1, x2 = v[..., 0:rot:2].clone(), v[..., 1:rot:2].clone()
    v[..., 0:rot:2] = x1 * c - x2 * s
    v[..., 1:rot:2] = x2 * c + x1 * s
    with pytest.raises(AssertionError):
        ec.check_rope(v.reshape(T, -1).to(BF16), heads, pos, cs, hd, "gptj")


# ---------------------------------------------------------------------------
# argmax
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("V", [8, 1000, 2056, 50257])
@pytest.mark.parametrize("R", [1, 5])
def test_argmax_criterion_accepts_first_rejects_last_index(V, R):
    x = ec.greedy_rows(V, R, seed=V + R)
    v = x.float()
    m = v.amax(dim=1, keepdim=True)
    first = (v == m).float().argmax(dim=1)  # first True
    ec.check_argmax(first, x, "first")
    last = V - 1 - (v == m).flip(1).float().argmax(dim=1)
    with pytest.raises(AssertionError):
        ec.check_argmax(last, x, "last-index tie-break")
    if R == 5:
        want = ec.ref_argmax(x)
        assert want[1] == (3 * V) // 4 and want[2] == 0 and want[3] == 0
        assert want[4] == V // 2


# ---------------------------------------------------------------------------
# LoRA
# ---------------------------------------------------------------------------
def _lora_f32(d, drop_rank_row=False):
    out = d["out"].clone()
    W = d["B"].shape[1]
    for t in range(out.shape[0]):
        s = int(d["idx"][t])
        if s < 0:
            continue
        y = (d["A"][s].float() @ d["x"][t].float()) * d["scale"][s]
        if drop_rank_row:
            y[-1] = 0
        c = d["col_off"]
        out[t, c : c + W] = (out[t, c : c + W].float()
                             + d["B"][s].float() @ y).to(BF16)
    return out


@pytest.mark.parametrize("name", sorted(ec.LORA_CASES))
def test_lora_slack_is_the_measured_one_and_criterion_discriminates(name):
    d, slack = ec.lora_case(name)
    args = (d["out"], d["x"], d["A"], d["B"], d["scale"], d["idx"], d["col_off"])
    dev = ec.lora_measured_deviation(*args)
    print(f"{name}: fp32 kernel-order deviation {dev:.3e}, slack {slack:.3e}")
    assert 4 * dev <= slack <= 4 * dev * 1.05 + 1e-12
    # the kernel-order evaluation and a differently ordered fp32 one pass
    ec.check_lora_bgmv(ec.lora_bgmv_fp32_kernel_order(*args).to(BF16),
                       d["out"], *args[1:], slack, name)
    ec.check_lora_bgmv(_lora_f32(d), d["out"], *args[1:], slack, name)
    if (d["idx"] >= 0).any():
        with pytest.raises(AssertionError):
            ec.check_lora_bgmv(_lora_f32(d, drop_rank_row=True), d["out"],
                               *args[1:], slack, name + " rank row dropped")
        # a write outside the column window
        spill = _lora_f32(d)
        t = int((d["idx"] >= 0).nonzero()[0])
        spill[t, d["col_off"] + d["B"].shape[1]] += 1
        with pytest.raises(AssertionError):
            ec.check_lora_bgmv(spill, d["out"], *args[1:], slack, name)
    else:
        touched = _lora_f32(d)
        touched[0, 0] += 1
        with pytest.raises(AssertionError):
            ec.check_lora_bgmv(touched, d["out"], *args[1:], slack, name)
