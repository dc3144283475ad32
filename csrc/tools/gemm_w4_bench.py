#!/usr/bin/env python3
"""int4 (W4A16) decode GEMM probe: the native int4 skinny kernel against the
bf16 kernels that serve decode without quantization.

For Llama-3-8B's four projection shapes at M in {1, 16, 64, 256} it times
  w4      ops.skinny_gemm_w4 (packed int4, group-128 bf16 scales + zeros)
  skinny  ops.skinny_gemm (bf16)
  linear  F.linear (bf16, hipBLASLt)
with warmed calls between hip events, --reps timed windows of --iters calls
each, and prints the median us per call with the min..max spread and the
effective weight bandwidth (weight bytes of that format / median time). Each
call of a timed window uses the next of several weight copies that together
exceed the 256 MiB Infinity Cache, so the weights come from HBM as they do
in a decode step that walks a whole model.

With --engine it also reports decode steps/s of an LLMEngine (--model) at
each --batches value with quantization None and "int4".

The driver starts one child process per GPU step, each under its own time
limit, and stops at the first one that fails. --md FILE writes the results
as markdown tables.
"""
import argparse
import json
import os
import statistics
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
IMPLS = ("w4", "skinny", "linear")
CACHE_BYTES = 256 << 20


def _time_us(fn, copies, iters, reps):
    """us per call of `reps` windows of `iters` calls, call i on weight copy
    i % n: (median, min, max)."""
    import torch

    n = len(copies)
    for i in range(max(n, 10)):
        fn(copies[i % n])
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(copies[i % n])
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def _w4_bytes(N, K):
    return N * K // 2 + N * (K // 128) * 3  # nibbles + bf16 scale + zero


def worker_gemm(M, iters, reps):
    import torch
    import torch.nn.functional as F

    from production_stack_amd import ops

    assert torch.cuda.is_available() and ops.HAVE_EXT
    for (N, K, name) in SHAPES:
        torch.manual_seed(N * 1009 + K)
        x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 8
        n4 = 2 * CACHE_BYTES // _w4_bytes(N, K) + 1
        n16 = 2 * CACHE_BYTES // (N * K * 2) + 1
        w16 = [torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
               for _ in range(n16)]
        q4 = [ops.int4_quantize_weight(w16[i % n16]) for i in range(n16)]
        # further copies of the packed tensors: the bytes matter, not the
        # values
        q4 += [tuple(t.clone() for t in q4[i % n16])
               for i in range(n4 - n16)]
        cell = {"M": M, "N": N, "K": K, "name": name}
        t = {
            "w4": _time_us(lambda w: ops.skinny_gemm_w4(x, *w), q4, iters,
                           reps),
            "skinny": _time_us(lambda w: ops.skinny_gemm(x, w), w16, iters,
                               reps),
            "linear": _time_us(lambda w: F.linear(x, w), w16, iters, reps),
        }
        for k, (med, lo, hi) in t.items():
            nbytes = _w4_bytes(N, K) if k == "w4" else N * K * 2
            cell[k + "_us"] = round(med, 2)
            cell[k + "_min_us"] = round(lo, 2)
            cell[k + "_max_us"] = round(hi, 2)
            cell[k + "_TBps"] = round(nbytes / med / 1e6, 3)
        print("CELL " + json.dumps(cell), flush=True)
        del w16, q4
        torch.cuda.empty_cache()


def worker_engine(model, quant, batch, tokens):
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
        quantization=None if quant == "bf16" else quant,
    )
    eng = LLMEngine(cfg, device="cuda")
    p = SamplingParams(max_tokens=tokens, temperature=0.0, ignore_eos=True)
    vocab = eng.model_cfg.vocab_size
    for i in range(batch):
        eng.add_request(
            f"r{i}", [(7 * i + j) % (vocab - 10) + 5 for j in range(64)], p)
    # prefill and the first decode steps are warm-up; the rest is timed in
    # windows of 32 steps for the spread
    steps, t0, rates = 0, None, []
    while eng.has_unfinished():
        eng.step()
        steps += 1
        if steps >= 8 and (steps - 8) % 32 == 0:
            torch.cuda.synchronize()
            now = time.perf_counter()
            if t0 is not None:
                rates.append(32 / (now - t0))
            t0 = now
    res = {"model": model, "quantization": quant, "batch": batch,
           "graphs": eng.runner.graphs is not None,
           "windows": len(rates),
           "steps_per_s": round(statistics.median(rates), 1),
           "min": round(min(rates), 1), "max": round(max(rates), 1)}
    print("ENGINE " + json.dumps(res), flush=True)


def _child(args, limit, sink):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable,
           os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    if r.returncode != 0:
        print(f"step {' '.join(args)} ended with status {r.returncode}; "
              "stopping", flush=True)
        sys.exit(1)
    for line in r.stdout.splitlines():
        for tag in ("CELL ", "ENGINE "):
            if line.startswith(tag):
                sink.append((tag.strip(), json.loads(line[len(tag):])))


def _markdown(results):
    out = ["| shape | M | w4 us (min..max) | bf16 skinny us (min..max) | "
           "hipBLASLt bf16 us (min..max) | w4 TB/s | w4 vs best bf16 |",
           "|---|---|---|---|---|---|---|"]
    for tag, c in results:
        if tag != "CELL":
            continue
        best = min(c["skinny_us"], c["linear_us"])
        out.append(
            f"| {c['name']} {c['N']}x{c['K']} | {c['M']} | "
            + " | ".join(
                f"{c[k + '_us']} ({c[k + '_min_us']}..{c[k + '_max_us']})"
                for k in IMPLS)
            + f" | {c['w4_TBps']} | {best / c['w4_us']:.2f}x |")
    eng = [c for tag, c in results if tag == "ENGINE"]
    if eng:
        out += ["", "| model | batch | weights | graphs | decode steps/s "
                "(min..max of 32-step windows) |", "|---|---|---|---|---|"]
        for c in eng:
            out.append(
                f"| {c['model']} | {c['batch']} | {c['quantization']} | "
                f"{c['graphs']} | {c['steps_per_s']} "
                f"({c['min']}..{c['max']}) |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", type=int, nargs="*", default=list(MS))
    ap.add_argument("--engine", action="store_true",
                    help="also time engine decode steps, bf16 vs int4")
    ap.add_argument("--model", default="llama-3-8b",
                    choices=["mini-llama", "llama-3-8b"])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--tokens", type=int, default=168)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed to each child process")
    ap.add_argument("--md", default=None,
                    help="write the result tables to this markdown file")
    ap.add_argument("--worker", choices=["gemm", "engine"])
    ap.add_argument("--m", type=int)
    ap.add_argument("--quant")
    ap.add_argument("--batch", type=int)
    a = ap.parse_args()
    if a.worker == "gemm":
        worker_gemm(a.m, a.iters, a.reps)
        return
    if a.worker == "engine":
        worker_engine(a.model, a.quant, a.batch, a.tokens)
        return
    results = []
    for M in a.ms:
        _child(["--worker", "gemm", "--m", str(M), "--iters", str(a.iters),
                "--reps", str(a.reps)], a.step_timeout, results)
    if a.engine:
        for batch in a.batches:
            for quant in ("bf16", "int4"):
                _child(["--worker", "engine", "--quant", quant,
                        "--model", a.model, "--batch", str(batch),
                        "--tokens", str(a.tokens)], a.step_timeout, results)
    if a.md:
        with open(a.md, "w") as f:
            f.write(_markdown(results))


if __name__ == "__main__":
    main()
