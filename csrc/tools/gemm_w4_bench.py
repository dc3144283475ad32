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

--tiled instead probes the prefill-sized kernel, csrc/gemm_w4_tiled.hip, on
the same four shapes at M in {64, ..., 4096}. Per cell it times
  tiled    ops.gemm_w4_tiled
  tiled1   the same kernel with one split forced (A/B of the split-K rule)
  dequant  ops.int4_dequant + gemm_policy.linear, what int4_linear runs
           above M = 256 without the tiled backend
  skinny   ops.skinny_gemm_w4, where M <= 256
  bf16     gemm_policy.linear alone on a pre-dequantized weight: the floor
           `dequant` cannot beat
The candidates alternate within each of the --reps rounds, one window each;
a window is sized to about 0.1 s of work from a calibration call. It prints
the median us with the min..max spread, and tiled's TFLOP/s as 2*M*N*K over
its median time.

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


TILED_MS = (64, 128, 256, 512, 1024, 2048, 4096)
TILED_IMPLS = ("tiled", "tiled1", "dequant", "skinny", "bf16")


def _time_alternating(cands, reps, window_s=0.1):
    """{name: (median, min, max) us per call}: `reps` rounds, in each one
    window per candidate in turn; fn(i) is call i of a candidate."""
    import torch

    def window(fn, iters):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(i)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / iters

    iters = {}
    for name, fn in cands.items():
        window(fn, 10)  # warm-up
        per_call = window(fn, 10)
        iters[name] = max(10, min(2000, int(window_s * 1e6 / per_call)))
    out = {name: [] for name in cands}
    for _ in range(reps):
        for name, fn in cands.items():
            out[name].append(window(fn, iters[name]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def worker_tiled(M, reps):
    import torch

    from production_stack_amd import _C, ops
    from production_stack_amd.ops import gemm_policy

    assert torch.cuda.is_available() and ops.HAVE_EXT
    for (N, K, name) in SHAPES:
        torch.manual_seed(N * 1009 + K)
        x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda") / 8
        # weight copies that together exceed the Infinity Cache, as above
        n4 = 2 * CACHE_BYTES // _w4_bytes(N, K) + 1
        n16 = 2 * CACHE_BYTES // (N * K * 2) + 1
        w = torch.randn(N, K, dtype=torch.bfloat16, device="cuda") / 8
        q = ops.int4_quantize_weight(w)
        del w
        q4 = [q] + [tuple(t.clone() for t in q) for _ in range(n4 - 1)]
        wd = ops.int4_dequant(*q)
        w16 = [wd] + [wd.clone() for _ in range(n16 - 1)]
        out = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        cands = {
            "tiled": lambda i: ops.gemm_w4_tiled(x, *q4[i % n4]),
            "tiled1": lambda i: _C.gemm_w4_tiled(out, x, *q4[i % n4],
                                                 split_k=False),
            "dequant": lambda i: gemm_policy.linear(
                x, ops.int4_dequant(*q4[i % n4])),
            "bf16": lambda i: gemm_policy.linear(x, w16[i % n16]),
        }
        if M <= 256:
            cands["skinny"] = lambda i: ops.skinny_gemm_w4(x, *q4[i % n4])
        # same inputs, same answer, before anything is timed
        want = gemm_policy.linear(x, wd).float()
        cands["tiled1"](0)
        for k, got in (("tiled", cands["tiled"](0)), ("tiled1", out)):
            err = float((got.float() - want).abs().max() / want.abs().max())
            assert err < 2.0 ** -6, (k, M, N, K, err)
        cell = {"M": M, "N": N, "K": K, "name": name,
                "splits": _C.gemm_w4_tiled_splits(M, N, K)}
        for k, (med, lo, hi) in _time_alternating(cands, reps).items():
            cell[k + "_us"] = round(med, 1)
            cell[k + "_min_us"] = round(lo, 1)
            cell[k + "_max_us"] = round(hi, 1)
        cell["tiled_TFLOPs"] = round(
            2 * M * N * K / cell["tiled_us"] / 1e6, 1)
        print("TILED " + json.dumps(cell), flush=True)
        del q4, w16, wd, q
        torch.cuda.empty_cache()


def _markdown_tiled(results):
    out = ["| shape | M | splits | tiled us (min..max) | one split us | "
           "dequant + bf16 us (min..max) | skinny w4 us | bf16 alone us | "
           "tiled TFLOP/s | dequant / tiled |",
           "|---|---|---|---|---|---|---|---|---|---|"]

    def span(c, k):
        if k + "_us" not in c:
            return "-"
        return f"{c[k + '_us']} ({c[k + '_min_us']}..{c[k + '_max_us']})"

    for tag, c in results:
        if tag != "TILED":
            continue
        out.append(
            f"| {c['name']} {c['N']}x{c['K']} | {c['M']} | {c['splits']} | "
            + " | ".join(span(c, k) for k in TILED_IMPLS)
            + f" | {c['tiled_TFLOPs']} | "
            f"{c['dequant_us'] / c['tiled_us']:.2f}x |")
    return "\n".join(out) + "\n"


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
        for tag in ("CELL ", "ENGINE ", "TILED "):
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
    ap.add_argument("--tiled", action="store_true",
                    help="probe gemm_w4_tiled against the dequant path "
                         "instead (M defaults to 64..4096)")
    ap.add_argument("--worker", choices=["gemm", "engine", "tiled"])
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
    if a.worker == "tiled":
        worker_tiled(a.m, a.reps)
        return
    results = []
    if a.tiled:
        for M in (a.ms if a.ms != list(MS) else TILED_MS):
            _child(["--worker", "tiled", "--m", str(M), "--reps",
                    str(a.reps)], a.step_timeout, results)
        if a.md:
            with open(a.md, "w") as f:
                f.write(_markdown_tiled(results))
        return
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
