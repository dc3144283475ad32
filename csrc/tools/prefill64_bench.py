#!/usr/bin/env python3
"""A/B of the head_dim-64 MFMA chunked-prefill kernel (csrc/prefill_mfma64.hip)
on an MI355X at Llama-3.2-1B attention shapes (32 q heads, 8 kv heads).

Per shape it times, alternating the three in every round:
  mfma64   paged_attn_prefill_mfma variant 5 at head_dim 64 (bf16 and fp8 KV)
  valu     paged_attn_prefill at head_dim 64, the only bf16 path before it
  v5@128   variant 5 at head_dim 128 with the same rows and contexts: exactly
           twice the FLOPs, so time(mfma64) / time(v5@128) = 0.5 would mean
           the D = 64 kernel is as MFMA-bound as v5
Times are device-event times per call, median over rounds of `iters` calls
after a warm-up of every kernel at every shape. FLOPs are 4 * hd * QH * (sum
of visible keys over rows), computed from the shape.

Prints one JSON line per shape; needs a GPU and fails without one.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", ".."))
import torch  # noqa: E402

from production_stack_amd import _C, ops  # noqa: E402

QH, KH, BS = 32, 8, 16
SHAPES = {  # name -> (num_seqs, history, rows)
    "fresh_1x1024": (1, 0, 1024),
    "fresh_8x512": (8, 0, 512),
    "cont_12x200_h4096": (12, 4096, 200),
}


def build(nseq, hist, rows, hd, fp8, seed=0):
    g = torch.Generator().manual_seed(seed)
    tile = ops.prefill_tile_rows(QH, KH)
    per = (hist + rows + BS - 1) // BS
    nb = nseq * per + 1
    k = torch.randn((nb, KH, BS, hd), generator=g).to(torch.bfloat16).cuda()
    v = torch.randn((nb, KH, BS, hd), generator=g).to(torch.bfloat16).cuda()
    if fp8:
        k, v = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
    bt = (torch.randperm(nseq * per, generator=g) + 1).to(torch.int32)
    bt = bt.reshape(nseq, per).cuda()
    T = nseq * rows
    q = torch.randn((T, QH, hd), generator=g).to(torch.bfloat16).cuda()
    tiles, seq, pos = [], [], []
    for s in range(nseq):
        for r0 in range(0, rows, tile):
            tiles.append([s, s * rows + r0, hist + r0, min(tile, rows - r0)])
        seq += [s] * rows
        pos += list(range(hist, hist + rows))
    i32 = dict(dtype=torch.int32, device="cuda")
    return dict(q=q, k=k, v=v, bt=bt, tiles=torch.tensor(tiles, **i32),
                seq=torch.tensor(seq, **i32), pos=torch.tensor(pos, **i32),
                out=torch.empty_like(q), scale=hd ** -0.5)


def mfma(a):
    _C.paged_attn_prefill_mfma(a["out"], a["q"], a["k"], a["v"], a["bt"],
                               a["tiles"], a["scale"], 5)


def valu(a):
    _C.paged_attn_prefill(a["out"], a["q"], a["k"], a["v"], a["bt"],
                          a["seq"], a["pos"], a["scale"], 0)


def timed(fn, a, iters):
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    for _ in range(iters):
        fn(a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def main(rounds=7, iters=100):
    assert torch.cuda.is_available(), "prefill64_bench needs a GPU"
    assert ops.prefill_mfma_supported(64)
    for name, (nseq, hist, rows) in SHAPES.items():
        runs = {
            "mfma64_bf16": (mfma, build(nseq, hist, rows, 64, False), iters),
            "mfma64_fp8": (mfma, build(nseq, hist, rows, 64, True), iters),
            "valu_bf16": (valu, build(nseq, hist, rows, 64, False),
                          max(2, iters // 10)),
            "v5_hd128_bf16": (mfma, build(nseq, hist, rows, 128, False),
                              iters),
        }
        # same inputs, both kernels: the A/B compares equal work
        a, b = runs["mfma64_bf16"][1], runs["valu_bf16"][1]
        mfma(a)
        valu(b)
        diff = (a["out"].float() - b["out"].float()).abs().max().item()
        for fn, arg, n in runs.values():  # warm-up
            timed(fn, arg, 2)
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, (fn, arg, n) in runs.items():
                ms[k].append(timed(fn, arg, n))
        keys = nseq * sum(hist + r + 1 for r in range(rows))
        res = {"shape": name, "max_abs_diff_mfma64_vs_valu": diff}
        for k, t in ms.items():
            med = statistics.median(t)
            hd = 128 if "128" in k else 64
            res[k] = {"ms": round(med, 4), "min_ms": round(min(t), 4),
                      "max_ms": round(max(t), 4),
                      "tflops": round(4 * hd * QH * keys / med / 1e9, 1)}
        res["valu_over_mfma64"] = round(
            res["valu_bf16"]["ms"] / res["mfma64_bf16"]["ms"], 2)
        res["mfma64_over_v5_hd128"] = round(
            res["mfma64_bf16"]["ms"] / res["v5_hd128_bf16"]["ms"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
