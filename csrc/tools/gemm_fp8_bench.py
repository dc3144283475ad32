#!/usr/bin/env python3
"""fp8 decode GEMM probe: the native fp8 skinny kernel against what serves
decode today.

For Llama-3-8B's four projection shapes at M in {1, 16, 64, 256} it times
  native   ops.skinny_gemm_fp8 (e4m3, row + channel scales)
  skinny   ops.skinny_gemm (bf16)
  scaledmm ops.fp8_linear with a per-tensor weight scale: torch act-quant
           (amax, divide, cast) + torch._scaled_mm, today's fp8 serving path
  linear   F.linear (bf16, hipBLASLt)
with warmed calls between hip events, and prints us per call and the
effective weight bandwidth (weight bytes of that format / time). Each call
of a timed window uses the next of several weight copies that together
exceed the 256 MiB Infinity Cache, so the weights come from HBM as they do
in a decode step that walks a whole model.

With --engine it also reports decode steps/s of an engine (mini-llama, or
--model llama-3-8b) under fp8_gemm=scaled_mm and fp8_gemm=native.

The driver starts one child process per GPU step, each under its own time
limit, and stops at the first one that fails.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

SHAPES = [  # (out_features, in_features) of Llama-3-8B's layer GEMMs
    (6144, 4096, "qkv"),
    (4096, 4096, "o"),
    (28672, 4096, "gate_up"),
    (4096, 14336, "down"),
]
MS = (1, 16, 64, 256)
IMPLS = ("native", "skinny", "scaledmm", "linear")
CACHE_BYTES = 256 << 20


def _time_us(fn, copies, iters):
    """Mean us per call over `iters` calls, call i on weight copy i % n."""
    import torch

    n = len(copies)
    for i in range(max(n, 10)):
        fn(copies[i % n])
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(copies[i % n])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def worker_gemm(M, iters):
    import torch
    import torch.nn.functional as F

    from production_stack_amd import ops

    assert torch.cuda.is_available() and ops.HAVE_EXT
    rows = []
    for (N, K, name) in SHAPES:
        torch.manual_seed(N * 1009 + K)
        x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 8
        xq, sx = ops.quant_fp8_rows(x)
        n8 = 2 * CACHE_BYTES // (N * K) + 1  # fp8 copies
        n16 = 2 * CACHE_BYTES // (N * K * 2) + 1
        w16 = [torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
               for _ in range(n16)]
        row_q = [ops.fp8_quantize_weight_rowwise(w16[i % n16])
                 for i in range(n8)]
        ten_q = [ops.fp8_quantize_weight(w16[i % n16]) for i in range(n8)]
        cell = {"M": M, "N": N, "K": K, "name": name}
        t = {
            "native": _time_us(
                lambda w: ops.skinny_gemm_fp8(xq, sx, w[0], w[1]),
                row_q, iters),
            "skinny": _time_us(lambda w: ops.skinny_gemm(x, w), w16, iters),
            "scaledmm": _time_us(
                lambda w: ops.fp8_linear(x, w[0], w[1]), ten_q, iters),
            "linear": _time_us(lambda w: F.linear(x, w), w16, iters),
        }
        for k, us in t.items():
            nbytes = N * K * (1 if k in ("native", "scaledmm") else 2)
            cell[k + "_us"] = round(us, 2)
            cell[k + "_TBps"] = round(nbytes / us / 1e6, 3)
        rows.append(cell)
        print("CELL " + json.dumps(cell), flush=True)
        del w16, row_q, ten_q
        torch.cuda.empty_cache()
    return rows


def worker_engine(model, backend, batch, tokens):
    import time

    import torch

    from production_stack_amd.engine.config import (
        CacheConfig,
        EngineConfig,
        SchedulerConfig,
    )
    from production_stack_amd.engine.engine import LLMEngine
    from production_stack_amd.engine.sampling import SamplingParams

    cfg = EngineConfig(
        model=model,
        max_model_len=2048,
        cache=CacheConfig(num_gpu_blocks=2048, block_size=16),
        scheduler=SchedulerConfig(max_num_seqs=batch,
                                  max_num_batched_tokens=4096),
        quantization="fp8",
        fp8_gemm=backend,
    )
    eng = LLMEngine(cfg, device="cuda")
    p = SamplingParams(max_tokens=tokens, temperature=0.0, ignore_eos=True)
    vocab = eng.model_cfg.vocab_size
    for i in range(batch):
        eng.add_request(
            f"r{i}", [(7 * i + j) % (vocab - 10) + 5 for j in range(64)], p)
    steps, t0 = 0, None
    while eng.has_unfinished():
        eng.step()
        steps += 1
        if steps == 8:  # prefill and the first decode steps are warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"model": model, "fp8_gemm": backend, "batch": batch,
           "graphs": eng.runner.graphs is not None,
           "decode_steps": steps - 8,
           "steps_per_s": round((steps - 8) / dt, 1)}
    print("ENGINE " + json.dumps(res), flush=True)


def _child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable,
           os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, cwd=ROOT)
    if r.returncode != 0:
        print(f"step {' '.join(args)} ended with status {r.returncode}; "
              "stopping", flush=True)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ms", type=int, nargs="*", default=list(MS))
    ap.add_argument("--engine", action="store_true",
                    help="also time engine decode steps under both backends")
    ap.add_argument("--model", default="mini-llama",
                    choices=["mini-llama", "llama-3-8b"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=136)
    ap.add_argument("--step-timeout", type=int, default=150,
                    help="seconds allowed to each child process")
    ap.add_argument("--worker", choices=["gemm", "engine"])
    ap.add_argument("--m", type=int)
    ap.add_argument("--backend")
    a = ap.parse_args()
    if a.worker == "gemm":
        worker_gemm(a.m, a.iters)
        return
    if a.worker == "engine":
        worker_engine(a.model, a.backend, a.batch, a.tokens)
        return
    for M in a.ms:
        _child(["--worker", "gemm", "--m", str(M), "--iters", str(a.iters)],
               a.step_timeout)
    if a.engine:
        for backend in ("scaled_mm", "native"):
            _child(["--worker", "engine", "--backend", backend,
                    "--model", a.model, "--batch", str(a.batch),
                    "--tokens", str(a.tokens)], a.step_timeout)


if __name__ == "__main__":
    main()
