"""gemm8p and skinny_gemm vs an fp64 reference, with the split-K workspace
poisoned.

Reference for every case: x.double() @ w.double().T as a GPU fp64 matmul
(hipBLAS dgemm, no in-tree kernel involved). Inputs follow the project's
randn/8 convention with a seed fixed per shape.

Tolerance: the project's existing GEMM bound atol = rtol = 3e-2
(tests/test_kernels_gpu.py::test_skinny_gemm), kept as is and not
tightened. With randn/8 operands the outputs have std sqrt(K)/64 (1.0 at
K=4096), so one bf16 output ulp (2^-7 relative) is well inside the bound,
while a dropped, doubled or misplaced 64-wide K-tile shifts every output it
touches by a value of std sqrt(64)/64 = 0.125 and is well outside it.
Errors a tolerance could still absorb -- a swizzle or fragment permutation
that pairs the wrong k indices -- are caught by the exact-integer cases,
which assert bit equality.

Both kernels run split-K through an fp32 workspace ws[splits, M, N] that the
binding allocates uninitialised and a combine kernel sums over all `splits`
slices. The poisoned cases fill exactly the block the caching allocator will
hand the binding with NaN first, so a slice no workgroup writes shows up as
NaN in the output instead of depending on what the memory held before.
"""

import pytest
import torch
import torch.nn.functional as F

from production_stack_amd import ops
from production_stack_amd.engine.config import ARCHITECTURES
from production_stack_amd.ops import gemm_policy

pytestmark = pytest.mark.gpu

TOL = 3e-2

# op name -> width of the K unit its split-K partition counts in
_UNIT = {"gemm8p": 128, "skinny": 64}

POISON_8P = [(16, 4096, 4096), (16, 4096, 14336), (300, 4096, 4096)]
POISON_SKINNY = [(16, 3072, 4096), (1, 6144, 768), (33, 2048, 5632)]

PATHS_8P = [
    # one tile, one K-pair: the prologue stages past kt_end
    (1, 256, 128),
    # full tile, two splits
    (256, 256, 256),
    # row clamp and the row<M guard
    (255, 256, 256), (257, 512, 256),
    # workgroup count not a multiple of 8 (6 and 18): XCD remap, wg>=nwg exit
    (300, 768, 640), (257, 2304, 384),
    # direct bf16 epilogue, splits == 1, odd K-pair count (196 workgroups)
    (1024, 12544, 384),
    # uneven but non-empty last split (4 splits of 2,2,2,1 K-pairs)
    (512, 12288, 896),
]
STRIDED_8P = (32, 512, 512)
EXACT_8P = (257, 512, 640)
EXACT_SKINNY = (129, 128, 192)
MTILE_SKINNY = [(M, 128, 192)
                for M in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)]
DISPATCH = (16, 512, 512)

SWEEP_M = (1, 16, 64, 256, 257, 512, 1024)


def setup_module(module):
    assert ops.HAVE_EXT, "HIP extension must be built on a GPU box"


def _C():
    from production_stack_amd import _C as ext

    return ext


def _op(name):
    return ops.gemm8p if name == "gemm8p" else ops.skinny_gemm


def _splits(name, M, N, K):
    ext = _C()
    fn = ext.gemm8p_splits if name == "gemm8p" else ext.skinny_gemm_splits
    return fn(M, N, K)


def _inputs(M, N, K, x_pad=0):
    torch.manual_seed(M * 1000003 + N * 1009 + K)
    x = torch.randn(M, K + x_pad, dtype=torch.bfloat16, device="cuda") / 8
    w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
    return x[:, :K], w


def _ref(x, w):
    return x.double() @ w.double().T


def _assert_matches(got, want):
    assert got.dtype == torch.bfloat16
    assert bool(torch.isfinite(got).all()), (
        f"{int((~torch.isfinite(got)).sum())}/{got.numel()} outputs are "
        "not finite"
    )
    torch.testing.assert_close(got.double(), want, atol=TOL, rtol=TOL)


# ---------------------------------------------------------------- (a) ----

def _poisoned_call(name, x, w):
    """Run the op with its split-K workspace landing on an all-NaN block."""
    M, K = x.shape
    N = w.shape[0]
    splits = _splits(name, M, N, K)
    assert splits > 1, "case must take the split-K workspace path"
    n = splits * M * N
    # keeps a block of the output's size free so the op's `out` allocation
    # (made before the workspace) cannot take the poisoned block
    spacer = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    poison = torch.full((n,), float("nan"), dtype=torch.float32,
                        device="cuda")
    ptr = poison.data_ptr()
    del poison
    again = torch.empty(n, dtype=torch.float32, device="cuda")
    # premise: an uninitialised allocation of the workspace's size gets the
    # NaN block back
    assert again.data_ptr() == ptr, "allocator did not reuse the block"
    assert bool(torch.isnan(again).all()), "reused block is not all-NaN"
    del again
    del spacer
    got = _op(name)(x, w)
    # the op's workspace is free again: the same request must lead back to
    # the poisoned block, now holding the first split's finite partials
    probe = torch.empty(n, dtype=torch.float32, device="cuda")
    assert probe.data_ptr() == ptr, "workspace did not use the NaN block"
    assert bool(torch.isfinite(probe[: M * N]).all()), (
        "split 0 of the workspace was not written"
    )
    del probe
    return got


@pytest.mark.parametrize(
    "name,M,N,K",
    [("gemm8p",) + s for s in POISON_8P]
    + [("skinny",) + s for s in POISON_SKINNY],
)
def test_poisoned_workspace(name, M, N, K):
    x, w = _inputs(M, N, K)
    want = _ref(x, w)
    runs = [_poisoned_call(name, x, w) for _ in range(3)]
    _assert_matches(runs[0], want)
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int16), runs[0].view(torch.int16)), (
            "repeated runs are not bit-identical"
        )


# ---------------------------------------------------------------- (b) ----

def _preset_shapes():
    """(N, K) of every projection of every model preset at TP 1, 2, 4, 8,
    sharded as engine/models/llama.py shards them."""
    shapes = set()
    for cfg in ARCHITECTURES.values():
        for tp in (1, 2, 4, 8):
            if cfg.num_q_heads % tp or cfg.intermediate_size % tp:
                continue
            if cfg.num_kv_heads % tp and tp % cfg.num_kv_heads:
                continue
            h = cfg.hidden_size
            qs = cfg.num_q_heads // tp * cfg.head_dim
            kvs = max(cfg.num_kv_heads // tp, 1) * cfg.head_dim
            inter = cfg.intermediate_size // tp
            shapes |= {
                (qs + 2 * kvs, h), (h, qs), (2 * inter, h), (h, inter),
                (cfg.vocab_size, h),
            }
    return sorted(shapes)


def _file_shapes():
    return (POISON_8P + POISON_SKINNY + PATHS_8P + MTILE_SKINNY
            + [STRIDED_8P, EXACT_8P, EXACT_SKINNY, DISPATCH])


@pytest.mark.parametrize("name", ["gemm8p", "skinny"])
def test_no_empty_split(name):
    """Host only. Restates the kernels' partition rule: split s covers units
    [s*per, min(units, (s+1)*per)) with per = ceil(units/splits), so the last
    split is non-empty iff per*(splits-1) < units. An empty split returns
    before writing its workspace slice, which the combine kernel still
    sums."""
    cases = {(M, N, K) for M in SWEEP_M for (N, K) in _preset_shapes()}
    cases |= set(_file_shapes())
    checked, bad = 0, []
    for (M, N, K) in sorted(cases):
        s = _splits(name, M, N, K)
        if s <= 0:
            continue
        checked += 1
        units = K // _UNIT[name]
        per = -(-units // s)
        if not per * (s - 1) < units:
            bad.append((M, N, K, s, per, -(-units // per)))
    assert checked > 100
    assert not bad, (
        f"{len(bad)}/{checked} shapes launch empty splits; first "
        f"(M, N, K, splits, per_split, non-empty): {bad[:8]}"
    )


# ---------------------------------------------------------------- (c) ----

@pytest.mark.parametrize("M,N,K", PATHS_8P)
def test_gemm8p_paths(M, N, K):
    """Back-to-back launches: a staged tile read before it has landed (a
    counted-vmcnt error) passes a lone cold call and shows once the previous
    launch keeps the memory system busy."""
    x, w = _inputs(M, N, K)
    want = _ref(x, w)
    runs = [ops.gemm8p(x, w) for _ in range(4)]
    for r in runs:
        _assert_matches(r, want)
        assert torch.equal(r.view(torch.int16), runs[0].view(torch.int16))


def test_gemm8p_strided_x():
    """x as a column slice of a wider buffer (row stride > K)."""
    M, N, K = STRIDED_8P
    x, w = _inputs(M, N, K, x_pad=512)
    assert x.stride(0) == K + 512 and not x.is_contiguous()
    _assert_matches(ops.gemm8p(x, w), _ref(x, w))


# ---------------------------------------------------------------- (d) ----

@pytest.mark.parametrize(
    "name,M,N,K", [("gemm8p",) + EXACT_8P, ("skinny",) + EXACT_SKINNY]
)
def test_exact_integer(name, M, N, K):
    """64 ones per x row and integer w in [-2, 2]: every partial sum is an
    integer of magnitude <= 128, exact in fp32 and in bf16, so the result
    must equal the integer reference bit for bit in any summation order."""
    g = torch.Generator(device="cuda").manual_seed(M * 1000003 + N * 1009 + K)
    cols = torch.rand(M, K, device="cuda", generator=g).argsort(1)[:, :64]
    x = torch.zeros(M, K, device="cuda")
    x.scatter_(1, cols, 1.0)
    assert bool((x.sum(1) == 64).all())
    w = torch.randint(-2, 3, (N, K), device="cuda", generator=g).float()
    want = _ref(x, w)
    assert float(want.abs().max()) <= 128
    got = _op(name)(x.to(torch.bfloat16), w.to(torch.bfloat16))
    assert torch.equal(got.double(), want), (
        f"{int((got.double() != want).sum())}/{want.numel()} outputs differ "
        "from the exact integer result"
    )


# ---------------------------------------------------------------- (e) ----

@pytest.mark.parametrize("M,N,K", MTILE_SKINNY)
def test_skinny_m_tiles(M, N, K):
    x, w = _inputs(M, N, K)
    _assert_matches(ops.skinny_gemm(x, w), _ref(x, w))


# ---------------------------------------------------------------- (f) ----

def _bf16(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16, device="cuda")


@pytest.mark.parametrize("M,N,K", [(16, 320, 128), (16, 256, 192)])
def test_gemm8p_rejects(M, N, K):
    with pytest.raises(RuntimeError):
        ops.gemm8p(_bf16(M, K), _bf16(N, K))


@pytest.mark.parametrize("M,N,K", [(257, 64, 64), (16, 96, 64), (16, 64, 96)])
def test_skinny_rejects(M, N, K):
    with pytest.raises(RuntimeError):
        ops.skinny_gemm(_bf16(M, K), _bf16(N, K))


@pytest.mark.parametrize("M,N,K", [(16, 0, 64), (16, 64, 0)])
def test_skinny_rejects_empty_dims(M, N, K):
    """Host only: N = 0 and K = 0 fail the accept rule before any launch."""
    assert _splits("skinny", M, N, K) == -1
    with pytest.raises(RuntimeError):
        ops.skinny_gemm(_bf16(M, K), _bf16(N, K))


@pytest.mark.parametrize("shape", [(16, 128), (32, 64), (16 * 64,)])
def test_skinny_rejects_out_shape(shape):
    """Host only: out must be [M, N], also where its element count fits."""
    M, N, K = 16, 64, 64
    with pytest.raises(RuntimeError):
        _C().skinny_gemm(_bf16(*shape), _bf16(M, K), _bf16(N, K))


def test_policy_eligibility_matches_kernels():
    """Host only: the autotuner offers a kernel exactly where it accepts."""
    dims = (32, 64, 96, 128, 192, 256, 320, 384, 512, 4096, 14336)
    for M in SWEEP_M:
        for N in dims:
            for K in dims:
                assert gemm_policy._eligible(M, N, K) == (
                    _splits("skinny", M, N, K) > 0), (M, N, K)
                assert gemm_policy._eligible_8p(M, N, K) == (
                    _splits("gemm8p", M, N, K) > 0), (M, N, K)


# ---------------------------------------------------------------- (g) ----

def test_policy_dispatch():
    M, N, K = DISPATCH
    x, w = _inputs(M, N, K)
    want = _ref(x, w)
    x2, w2 = _inputs(24, 384, 320)  # no policy entry
    try:
        for impl in (1, 2):
            gemm_policy._POLICY[(M, N, K)] = impl
            _assert_matches(gemm_policy.linear(x, w), want)
            assert torch.equal(gemm_policy.linear(x2, w2), F.linear(x2, w2))
    finally:
        gemm_policy.reset()
    assert not gemm_policy._POLICY
