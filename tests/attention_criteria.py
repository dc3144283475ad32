"""fp64 reference, rounding model, pass criterion and mutants for the
chunked-prefill attention kernels (paged_attn_prefill_mfma variants 5 and 3,
paged_attn_prefill).

Everything here is plain torch on the CPU and independent of
production_stack_amd.ops.reference and of any GPU kernel.
tests/test_attention_criteria_cpu.py shows that the criterion accepts an
honest fp32 evaluation and the rounding model itself and rejects every
mutant below on every case of CASES; tests/test_prefill_edges_gpu.py applies
the same criterion to the kernels on the same cases.

The criterion, per output element of row t and head h:

    |got - exact| <= 1.01 * half_ulp_bf16(exact) + F * dev[t, h]

`exact` is causal (optionally windowed) softmax attention in fp64 over the
keys gathered through the block table. `dev[t, h]` is the largest
|model - exact| over the head dimension, where `model` is the same
computation with the intermediate roundings the kernel makes and nothing
else, taken before the final rounding to bf16:

  MFMA kernels (csrc/prefill_mfma32.hip, csrc/prefill_mfma.hip)
    * q * (scale * log2 e) rounded to bf16 before QK^T
    * P rounded to bf16 before PV, divided by the unrounded row sum. P is
      2^(score - m_run), and defer-max lets m_run lag the row's maximum by
      up to 8 nats, so a dominant P is not 1 and does round; the model walks
      the 64-key chunks, per split, with the kernels' rescale rule
      (_online_softmax)
  VALU kernel (csrc/attention.hip, paged_attn_prefill_kernel)
    makes neither: q * scale, the scores, P and the accumulators stay in
    fp32. Its model is the whole expression evaluated in fp32, so its dev
    is fp32 noise and the bound is in effect one bf16 rounding.

F = 2: the kernel is another draw from the same error process (its scores
are fp32 sums in another order, so a rescale decision near the threshold can
fall the other way; splits merge fp32 partials) and dev is already the
maximum of hd draws. dev is per row
and head on purpose: a slack global to a case is set by its shortest rows
and hides the long ones.

A criterion raises AssertionError and otherwise returns its worst figure in
units of its bound, so a caller can print it.
"""

from __future__ import annotations

import dataclasses
import functools
from typing import Optional

import torch

from tests.elementwise_criteria import MARGIN, half_ulp_bf16

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn

BS = 16       # page size in tokens
KH = 2
CHUNK = 64    # KV tokens the MFMA kernels consume per step
F = 2.0
LOG2E_F32 = 1.44269504  # the literal both MFMA kernels multiply scale by
LOUD_V = {False: 1024.0, True: 448.0}  # e4m3 tops out at 448


# ---------------------------------------------------------------------------
# case builder
# ---------------------------------------------------------------------------
def gqw(gq: int) -> int:
    """Q heads per variant-5 workgroup: largest power-of-two divisor of the
    GQA ratio, at most 4."""
    w = 1
    while w < 4 and gq % (w * 2) == 0:
        w *= 2
    return w


def v5_tile_rows(gq: int) -> int:
    return 32 * (8 // gqw(gq))


def v5_splits(num_tiles: int, kh: int, gq: int) -> int:
    """The split count variant 5 documents: ~500 workgroups, at most 8."""
    n_work = num_tiles * kh * (gq // gqw(gq))
    if n_work >= 500:
        return 1
    return min(8, -(-500 // n_work))


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    q: torch.Tensor           # [T, QH, hd] bf16
    k: torch.Tensor           # [NB+1, KH, 16, hd] bf16 or e4m3
    v: torch.Tensor
    bt: torch.Tensor          # [S, max_blocks] int32, padding -> block NB
    tiles: torch.Tensor       # [NT, 4] int32 (seq_row, q_tok0, q_pos0, n)
    token_seq: torch.Tensor   # [T] int32
    token_pos: torch.Tensor   # [T] int32
    chunks: tuple             # ((seq_row, start_pos, n_tokens), ...)
    seq_len: tuple            # final position + 1 of every sequence
    scale: float
    hd: int
    gq: int

    @property
    def qh(self):
        return KH * self.gq

    def k64(self):
        return self.k.to(F32).to(F64)

    def v64(self):
        return self.v.to(F32).to(F64)


def build_case(seed, hd, gq, chunks, tile_rows, peaked=False, fp8=False):
    """Seeded inputs for one call. Block tables are a shuffled,
    non-contiguous subset of the cache; table entries past a sequence's
    last page point at block NB, which is all NaN; the slots of a last page
    beyond the sequence's final position hold finite loud values (V = 1024,
    or 448 in an fp8 cache; K = 8 x randn), because the MFMA kernels
    legitimately multiply p = 0 by those V rows. `peaked` multiplies each
    sequence's first key and the key at each tile's last position by 8."""
    chunks = tuple(tuple(c) for c in chunks)
    S = 1 + max(c[0] for c in chunks)
    seq_len = [0] * S
    for s, start, n in chunks:
        assert n > 0 and start >= 0
        seq_len[s] = max(seq_len[s], start + n)
    pages = [-(-n // BS) for n in seq_len]
    NB = sum(pages) + 8  # a few blocks no table uses
    g = torch.Generator().manual_seed(seed)
    k = torch.randn((NB + 1, KH, BS, hd), generator=g)
    v = torch.randn((NB + 1, KH, BS, hd), generator=g)
    loud = torch.randn((S, KH, BS, hd), generator=g) * 8.0
    bt = torch.full((S, max(pages) + 2), NB, dtype=torch.int32)
    perm = torch.randperm(NB, generator=g).to(torch.int32)
    used = 0
    for s in range(S):
        bt[s, :pages[s]] = perm[used:used + pages[s]]
        used += pages[s]
        tail = seq_len[s] % BS
        if tail:
            last = int(bt[s, pages[s] - 1])
            k[last, :, tail:] = loud[s, :, tail:]
            v[last, :, tail:] = LOUD_V[fp8]
    tiles, token_seq, token_pos = [], [], []
    peaks = {(s, 0) for s in range(S)}
    t = 0
    for s, start, n in chunks:
        for r0 in range(0, n, tile_rows):
            rows = min(tile_rows, n - r0)
            tiles.append([s, t + r0, start + r0, rows])
            peaks.add((s, start + r0 + rows - 1))
        token_seq += [s] * n
        token_pos += list(range(start, start + n))
        t += n
    if peaked:
        for s, p in sorted(peaks):
            k[int(bt[s, p // BS]), :, p % BS] *= 8.0
    k[NB] = float("nan")
    v[NB] = float("nan")
    k, v = k.to(BF16), v.to(BF16)
    if fp8:
        k, v = k.to(FP8), v.to(FP8)
        assert torch.isfinite(k[:NB].to(F32)).all()
        assert torch.isfinite(v[:NB].to(F32)).all()
    q = torch.randn((t, KH * gq, hd), generator=g).to(BF16)
    return Case(q=q, k=k, v=v, bt=bt,
                tiles=torch.tensor(tiles, dtype=torch.int32),
                token_seq=torch.tensor(token_seq, dtype=torch.int32),
                token_pos=torch.tensor(token_pos, dtype=torch.int32),
                chunks=chunks, seq_len=tuple(seq_len),
                scale=1.0 / hd ** 0.5, hd=hd, gq=gq)


# ---------------------------------------------------------------------------
# attention on the CPU: exact, rounding models, mutants
# ---------------------------------------------------------------------------
def _bf16_round(x64):
    return x64.to(F32).to(BF16).to(F64)


RESCALE_THR = 11.54  # PS_RESCALE_THR32 / PS_RESCALE_THR: 8 nats in log2 units


def _online_softmax(sc, valid, V, pos, wave_rows, n_splits, skip_last):
    """The MFMA kernels' walk over 64-key chunks, in fp64 except that P is
    rounded to bf16 before PV: sc [QH, n, Lk] exp2-domain scores, valid
    [n, Lk], V [QH, Lk, hd], pos [n, 1]. P is rounded against the running
    max m_run, which defer-max lets lag: m_run moves only when some row of
    the wave (`wave_rows` consecutive rows of one head) sees its max grow by
    more than RESCALE_THR, or meets its first key. Split s of n_splits walks
    chunks s, s + n_splits, ... and the partials are merged unrounded.
    Returns (o [QH, n, hd], rescaled_last [QH, n]): the latter marks rows
    whose accumulators were rescaled (by a factor other than 1, with keys
    already summed) in the chunk that holds their diagonal; with
    `skip_last` exactly those rescales are left out."""
    QH, n, Lk = sc.shape
    ninf = torch.tensor(float("-inf"), dtype=F64)
    wave = torch.arange(n) // wave_rows
    same_wave = (wave[:, None] == wave[None, :]).to(F64)
    last_chunk = pos // CHUNK  # [n, 1]
    rescaled_last = torch.zeros((QH, n), dtype=torch.bool)
    M = torch.full((QH, n, 1), float("-inf"), dtype=F64)
    parts = []
    for s in range(n_splits):
        m_run = torch.full((QH, n, 1), float("-inf"), dtype=F64)
        l_run = torch.zeros((QH, n, 1), dtype=F64)
        acc = torch.zeros((QH, n, V.shape[2]), dtype=F64)
        for c in range(s, -(-Lk // CHUNK), n_splits):
            sl = slice(c * CHUNK, min(Lk, (c + 1) * CHUNK))
            ok = valid[:, sl]
            if not ok.any():
                continue
            x = torch.where(ok, sc[:, :, sl], ninf)
            m_new = torch.maximum(m_run, x.amax(dim=2, keepdim=True))
            grew = (m_new > m_run + RESCALE_THR) | \
                (torch.isinf(m_run) & ~torch.isinf(m_new))
            any_grew = (grew[:, :, 0].to(F64) @ same_wave) > 0  # [QH, n]
            corr = torch.where(torch.isinf(m_new), torch.ones_like(m_new),
                               torch.exp2(m_run - m_new))
            moved = any_grew[:, :, None] & (corr != 1.0) & (l_run > 0)
            at_last = moved & (last_chunk == c)[None]
            rescaled_last |= at_last[:, :, 0]
            apply = any_grew[:, :, None]
            if skip_last:
                scale_by = torch.where(apply & ~at_last, corr,
                                       torch.ones_like(corr))
            else:
                scale_by = torch.where(apply, corr, torch.ones_like(corr))
            l_run = l_run * scale_by
            acc = acc * scale_by
            m_run = torch.where(apply, m_new, m_run)
            p = torch.where(ok, torch.exp2(x - m_run), torch.zeros_like(x))
            l_run = l_run + p.sum(dim=2, keepdim=True)
            acc = acc + _bf16_round(p) @ V[:, sl]
        parts.append((m_run, l_run, acc))
        M = torch.maximum(M, m_run)
    num = torch.zeros_like(parts[0][2])
    den = torch.zeros_like(parts[0][1])
    for m_run, l_run, acc in parts:
        w = torch.where(torch.isinf(m_run), torch.zeros_like(m_run),
                        torch.exp2(m_run - M))
        num += w * acc
        den += w * l_run
    return num / den, rescaled_last


def attend(case: Case, window: int = 0, mode: str = "exact", *,
           wave_rows: int = 32, n_splits: int = 1, rescaled_last=None,
           causal_shift: int = 0, window_shift: int = 0,
           drop_key: Optional[int] = None, swap_pages: bool = False,
           head_reads: Optional[tuple] = None, skip_last_rescale: bool = False,
           drop_split: Optional[tuple] = None):
    """[T, QH, hd] float64, before any final rounding.

    mode: "exact" (fp64), "mfma" (the bf16 roundings of the MFMA kernels,
    see _online_softmax; wave_rows is 32 for variant 5 and 16 for variant
    3, n_splits the split count the call runs; a [T, QH] bool tensor given
    as `rescaled_last` receives that function's second result), "fp32" (the
    VALU kernel: everything in fp32).

    The keyword arguments turn it into a subtly wrong kernel (see MUTANTS):
      causal_shift     key kv is visible when kv <= q + causal_shift
      window_shift     ... and kv > q - window + window_shift
      drop_key         this key position is invisible
      swap_pages       every sequence's first and last page swap places
      head_reads       (q_head, kv_head): that q head reads that kv head
      skip_last_rescale  the accumulators are not rescaled when the running
                       max grows in a row's last 64-token chunk ("mfma")
      drop_split       (n_splits, j): the keys of chunks j, j + n_splits, ...
                       are left out (split j's partial misses the merge)
    """
    T, QH, hd = case.q.shape
    k64, v64 = case.k64(), case.v64()
    kv_of = torch.arange(QH) // case.gq
    if head_reads is not None:
        kv_of[head_reads[0]] = head_reads[1]
    out = torch.empty((T, QH, hd), dtype=F64)
    qmul = (torch.tensor(case.scale, dtype=F32) *
            torch.tensor(LOG2E_F32, dtype=F32))
    t0 = 0
    for s, start, n in case.chunks:
        L = start + n
        npages = -(-(L + max(causal_shift, 0)) // BS)
        pages = case.bt[s, :npages].long().clone()
        if swap_pages:
            last = -(-case.seq_len[s] // BS) - 1
            if 0 < last < npages:
                pages[0], pages[last] = pages[last].clone(), pages[0].clone()
            elif last >= npages:
                pages[0] = case.bt[s, last]
        # [QH, Lk, hd]
        K = k64[pages].permute(1, 0, 2, 3).reshape(KH, -1, hd)[kv_of]
        V = v64[pages].permute(1, 0, 2, 3).reshape(KH, -1, hd)[kv_of]
        Lk = K.shape[1]
        pos = torch.arange(start, L)[:, None]
        kv = torch.arange(Lk)[None, :]
        valid = kv <= pos + causal_shift
        if window > 0:
            valid &= kv > pos - window + window_shift
        if drop_key is not None:
            valid &= kv != drop_key
        if drop_split is not None:
            valid &= (kv // CHUNK) % drop_split[0] != drop_split[1]
        qc = case.q[t0:t0 + n].permute(1, 0, 2)  # [QH, n, hd]
        if mode == "fp32":
            qs = qc.to(F32) * torch.tensor(case.scale, dtype=F32)
            sc = torch.where(valid, qs @ K.to(F32).transpose(1, 2),
                             torch.tensor(float("-inf"), dtype=F32))
            m = sc.amax(dim=2, keepdim=True)
            p = torch.where(valid, torch.exp(sc - m), torch.zeros_like(sc))
            o = (p @ V.to(F32)) / p.sum(dim=2, keepdim=True)
            o = o.to(F64)
        elif mode == "exact":
            sc = (qc.to(F64) @ K.transpose(1, 2)) * case.scale
            sc = torch.where(valid, sc, torch.tensor(float("-inf"), dtype=F64))
            m = sc.amax(dim=2, keepdim=True)
            p = torch.where(valid, torch.exp(sc - m), torch.zeros_like(sc))
            o = (p @ V) / p.sum(dim=2, keepdim=True)
        else:
            assert mode == "mfma", mode
            qs = (qc.to(F32) * qmul).to(BF16).to(F64)  # the kernel's own ops
            sc = qs @ K.transpose(1, 2)  # exp2 domain
            o, resc = _online_softmax(sc, valid, V, pos, wave_rows, n_splits,
                                      skip_last_rescale)
            if rescaled_last is not None:
                rescaled_last[t0:t0 + n] = resc.T
        # a row with no visible key: the kernels store 0
        none = ~valid.any(dim=1)
        o[:, none] = 0.0
        out[t0:t0 + n] = o.permute(1, 0, 2)
        t0 += n
    return out


# ---------------------------------------------------------------------------
# criterion
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Yardstick:
    exact: torch.Tensor   # [T, QH, hd] float64
    dev: torch.Tensor     # [T, QH] float64
    model: torch.Tensor   # [T, QH, hd] float64, unrounded


def yardstick(case: Case, window: int = 0, model: str = "mfma",
              **model_kw) -> Yardstick:
    """model_kw: wave_rows and n_splits of the "mfma" model."""
    exact = attend(case, window, "exact")
    mod = attend(case, window, model, **model_kw)
    assert torch.isfinite(exact).all() and torch.isfinite(mod).all()
    return Yardstick(exact, (mod - exact).abs().amax(dim=2), mod)


def error_over_bound(got, ys: Yardstick, f: float = F):
    """[T, QH, hd] float64; inf where got is not finite."""
    assert got.dtype == BF16, got.dtype
    g = got.detach().cpu().to(F64)
    assert g.shape == ys.exact.shape, (g.shape, ys.exact.shape)
    bound = half_ulp_bf16(ys.exact) * MARGIN + f * ys.dev[:, :, None]
    err = (g - ys.exact).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    return err / bound


def check(got, ys: Yardstick, what: str = "", f: float = F) -> float:
    ratio = error_over_bound(got, ys, f)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ratio > 1.0
    if bad.any():
        rows = int(bad.any(dim=2).any(dim=1).sum())
        t, h, d = [int(i) for i in
                   torch.unravel_index(ratio.argmax(), ratio.shape)]
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} elements in {rows} rows "
            f"beyond the bound; worst {worst:.3f}x at row {t} head {h} dim "
            f"{d}: got {float(got[t, h, d])!r} exact "
            f"{float(ys.exact[t, h, d])!r} dev {float(ys.dev[t, h])!r}")
    return worst


def rejected_pairs(got, ys: Yardstick, f: float = F):
    """[T, QH] bool: some element of that row and head is beyond the bound."""
    return (error_over_bound(got, ys, f) > 1.0).any(dim=2)


# ---------------------------------------------------------------------------
# mutants: name -> (kwargs for attend, touched [T, QH] bool) or None when the
# mutant does not apply to the case
# ---------------------------------------------------------------------------
def _all(case):
    return torch.ones((case.q.shape[0], case.qh), dtype=torch.bool)


def _rows(case, mask_t):
    return mask_t[:, None].expand(-1, case.qh).clone()


def mutants(case: Case, window: int, model: str, peaked: bool, splits: int,
            wave_rows: int = 32):
    """{name: (attend kwargs, touched)}. `touched` marks the (row, head)
    pairs whose visible keys, or their weights, the mutant changes."""
    pos = case.token_pos.long()
    seq = case.token_seq.long()
    slen = torch.tensor(case.seq_len)[seq]
    out = {}
    out["causal_lt"] = (dict(causal_shift=-1), _all(case))
    out["causal_le_q_plus_1"] = (dict(causal_shift=1), _all(case))
    if window > 0 and (pos >= window).any():
        out["window_lo_minus_1"] = (dict(window_shift=-1),
                                    _rows(case, pos >= window))
    if window > 0 and (pos >= window - 1).any():
        out["window_lo_plus_1"] = (dict(window_shift=1),
                                   _rows(case, pos >= window - 1))
    sees63 = pos >= CHUNK - 1
    if window > 0:
        sees63 &= (CHUNK - 1) > pos - window
    if sees63.any():
        out["drop_key_63"] = (dict(drop_key=CHUNK - 1), _rows(case, sees63))
    last_page = (slen - 1) // BS
    lo = torch.clamp(pos - window + 1, min=0) if window > 0 \
        else torch.zeros_like(pos)
    # one of the two pages is in sight, and not both of them whole
    swapped = (last_page > 0) & ((lo < BS) | (pos >= last_page * BS)) & \
        ~((lo == 0) & (pos == last_page * BS + BS - 1))
    if swapped.any():
        out["swap_first_and_last_page"] = (dict(swap_pages=True),
                                           _rows(case, swapped))
    touched = torch.zeros((case.q.shape[0], case.qh), dtype=torch.bool)
    touched[:, 0] = True
    out["q_head_0_reads_kv_head_1"] = (dict(head_reads=(0, 1)), touched)
    if peaked and model == "mfma":
        grows = torch.zeros((case.q.shape[0], case.qh), dtype=torch.bool)
        attend(case, window, "mfma", wave_rows=wave_rows, n_splits=splits,
               rescaled_last=grows)
        assert grows.any(), "a peaked case must rescale in a last chunk"
        out["skip_last_rescale"] = (dict(skip_last_rescale=True), grows)
    if splits > 1:
        lo = torch.clamp(pos - window + 1, min=0) if window > 0 \
            else torch.zeros_like(pos)
        c = torch.arange(int(pos.max()) // CHUNK + 1)[None, :]
        in_sight = (c >= lo[:, None] // CHUNK) & (c <= pos[:, None] // CHUNK)
        hit = (in_sight & (c % splits == 1)).any(dim=1)
        if hit.any():
            out["split_1_left_out"] = (dict(drop_split=(splits, 1)),
                                       _rows(case, hit))
    return out


# ---------------------------------------------------------------------------
# the case matrix, shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------
def edge_chunks(tile_rows, cap=None):
    """A fresh prompt one row longer than a tile; 70 rows from position 100
    (no multiple of 16, 32 or 64); a continuation ending exactly on a chunk
    edge; 1-token chunks at 0 and 63; a 5-row speculative-verification chunk
    at 1000 (at `cap` - 5 when contexts are capped)."""
    far = 1000 if cap is None else cap - 5
    return ((0, 0, tile_rows + 1), (1, 100, 70), (2, 200, 56), (3, 0, 1),
            (4, 63, 1), (5, far, 5))


def scattered_chunks(n, rows=3):
    """n chunks of `rows` rows, six to a sequence, at starts that are no
    multiple of anything."""
    starts = (0, 61, 125, 190, 333, 640)
    return tuple((c // 6, starts[c % 6] + 7 * (c // 6), rows)
                 for c in range(n))


def many_tiles(n, rows=2):
    """n chunks of `rows` rows, fifty to a sequence, 13 positions apart:
    enough tiles for variant 5 to run one split at a small GQ."""
    return tuple((c // 50, 13 * (c % 50) + c // 50, rows) for c in range(n))


SERVING = ((0, 1000, 5), (1, 2000, 64), (2, 256, 300))  # all contexts >= 256
TWO_TILES = ((0, 100, 50), (1, 0, 40))
# the same and two tiles whose contexts span more than 8 chunks, so that a
# split that already holds keys meets the peak in the row's last chunk
FOUR_TILES = TWO_TILES + ((2, 600, 60), (3, 900, 20))
WINDOW_OWN = ((0, 0, 130), (1, 100, 70), (2, 570, 70), (3, 63, 1))
WINDOWS = (1, 16, 63, 64, 65, 200, 5000)


@dataclasses.dataclass(frozen=True)
class Spec:
    kernel: str            # "v5", "v3" or "valu"
    gq: int
    chunks: tuple
    hd: int = 128
    fp8: bool = False
    peaked: bool = False
    window: int = 0
    splits: Optional[int] = None  # variant 5: the count the case must run

    @property
    def tile_rows(self):
        return v5_tile_rows(self.gq) if self.kernel == "v5" else 64

    @property
    def model(self):
        return "fp32" if self.kernel == "valu" else "mfma"

    @property
    def wave_rows(self):
        return 32 if self.kernel == "v5" else 16


def _specs():
    c = {}
    # variant 5: every instantiation on the edge chunks
    for gq in (1, 2, 3, 4, 6, 7, 8):
        c[f"v5_gq{gq}_bf16"] = Spec("v5", gq, edge_chunks(v5_tile_rows(gq)))
    for gq in (1, 2, 4):
        c[f"v5_gq{gq}_fp8"] = Spec("v5", gq, edge_chunks(v5_tile_rows(gq)),
                                   fp8=True)
    # split counts on purpose
    c["v5_splits1"] = Spec("v5", 7, scattered_chunks(36), splits=1)
    c["v5_splits2"] = Spec("v5", 7, scattered_chunks(18), splits=2)
    c["v5_splits3"] = Spec("v5", 7, scattered_chunks(12), splits=3)
    c["v5_splits5"] = Spec("v5", 6, scattered_chunks(18), splits=5)
    c["v5_splits8"] = Spec("v5", 4, TWO_TILES, splits=8)
    # serving contexts: the shapes at which a 2e-2 tolerance sees nothing
    c["v5_serving"] = Spec("v5", 4, SERVING)
    c["v5_serving_w200"] = Spec("v5", 4, SERVING, window=200)
    # peaked softmax at 1 split and at 8
    c["v5_peaked_gq4_s1"] = Spec("v5", 4, many_tiles(250), peaked=True,
                                 splits=1)
    c["v5_peaked_gq4_s8"] = Spec("v5", 4, FOUR_TILES, peaked=True,
                                 splits=8)
    c["v5_peaked_gq7_s1"] = Spec("v5", 7, scattered_chunks(36), peaked=True,
                                 splits=1)
    c["v5_peaked_gq7_s8"] = Spec("v5", 7, FOUR_TILES, peaked=True,
                                 splits=8)
    # sliding window
    for w in WINDOWS:
        for gq in (2, 4):
            c[f"v5_w{w}_gq{gq}_s1"] = Spec("v5", gq, many_tiles(250),
                                           window=w, splits=1)
            c[f"v5_w{w}_gq{gq}_own"] = Spec("v5", gq, WINDOW_OWN, window=w,
                                            splits=8)
    c["v5_w65_gq4_fp8"] = Spec("v5", 4, WINDOW_OWN, window=65, fp8=True,
                               splits=8)
    # variant 3
    for gq in (1, 4, 7):
        c[f"v3_gq{gq}_bf16"] = Spec("v3", gq, edge_chunks(64))
        c[f"v3_gq{gq}_fp8"] = Spec("v3", gq, edge_chunks(64), fp8=True)
    c["v3_serving"] = Spec("v3", 4, SERVING)
    c["v3_peaked"] = Spec("v3", 4, edge_chunks(64), peaked=True)
    for w in (1, 64, 65):
        c[f"v3_w{w}"] = Spec("v3", 4, WINDOW_OWN, window=w)
    # VALU kernel: head_dim 64 (GQ is a run-time argument there: the ratios
    # the decode dispatcher knows for head_dim 64, and an odd one), and
    # head_dim 128 with GQ 4
    for hd, gq in ((64, 1), (64, 2), (64, 3), (64, 4), (64, 8), (128, 4)):
        for w in (0, 1, 17):
            c[f"valu_hd{hd}_gq{gq}_w{w}"] = Spec(
                "valu", gq, edge_chunks(64, cap=300), hd=hd, window=w)
    return c


CASES = _specs()


@functools.lru_cache(maxsize=None)
def _case_of(kernel, hd, gq, chunks, tile_rows, peaked, fp8):
    seed = 7919 * hd + 31 * gq + 1009 * len(chunks) + 17 * peaked + 3 * fp8 \
        + sum(c[1] + c[2] for c in chunks)
    return build_case(seed, hd, gq, chunks, tile_rows, peaked, fp8)


def case(name) -> Case:
    """The seeded inputs of a CASES entry, built once and never modified
    (cases that differ only in the window share them)."""
    s = CASES[name]
    return _case_of(s.kernel, s.hd, s.gq, s.chunks, s.tile_rows, s.peaked,
                    s.fp8)


@functools.lru_cache(maxsize=None)
def _yardstick_of(kernel, hd, gq, chunks, tile_rows, peaked, fp8, window,
                  model, wave_rows, n_splits):
    kw = dict(wave_rows=wave_rows, n_splits=n_splits) if model == "mfma" \
        else {}
    return yardstick(_case_of(kernel, hd, gq, chunks, tile_rows, peaked, fp8),
                     window, model, **kw)


def case_yardstick(name) -> Yardstick:
    s = CASES[name]
    return _yardstick_of(s.kernel, s.hd, s.gq, s.chunks, s.tile_rows,
                         s.peaked, s.fp8, s.window, s.model, s.wave_rows,
                         expected_splits(name))


def expected_splits(name) -> int:
    """The split count the case runs: variant 5's rule, 1 elsewhere."""
    s = CASES[name]
    if s.kernel != "v5":
        return 1
    return v5_splits(case(name).tiles.shape[0], KH, s.gq)


def model_kw(name) -> dict:
    """attend()'s keyword arguments for the case's rounding model."""
    s = CASES[name]
    if s.model != "mfma":
        return {}
    return dict(wave_rows=s.wave_rows, n_splits=expected_splits(name))


def min_context(name) -> int:
    return int(case(name).token_pos.min()) + 1
