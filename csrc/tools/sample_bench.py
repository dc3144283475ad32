#!/usr/bin/env python3
"""Sampler probe: ops.sample (csrc/sample.hip) against the torch path.

For V in {32000, 128256, 152064}, R in {1, 16, 256} and four filter sets
(none / top-k 50 / top-p 0.9 / top-k + top-p + min-p, all at temperature 0.8)
it times, in one process per V,
  kernel  ops.sample alone: records already on the device, back-to-back
          launches
  native  ModelRunner.sample_params under sampler="native": pack the records,
          upload, one launch, .cpu() of the [R] result
  torch   ModelRunner.sample_params under sampler="torch", what these rows run
          without the native sampler: torch ops on the device, the [R, V]
          probabilities copied to the host, multinomial there
native and torch end in a device-to-host copy, so every window is timed with
a host clock around calls that end in a device synchronise; the candidates
alternate within each of the --reps rounds, one window
each, a window sized to about 0.1 s from a calibration call (3 calls at
least). Each call reads the next of several logits copies (up to 8, together
above the 256 MiB Infinity Cache where 8 suffice). It prints the median us
with the min..max spread; --md FILE writes the table as markdown.

The driver starts one child process per V, each under its own time limit, and
stops at the first one that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

VS = (32000, 128256, 152064)
RS = (1, 16, 256)
FILTERS = {  # name -> (top_k, top_p, min_p)
    "none": (-1, 1.0, 0.0),
    "top-k 50": (50, 1.0, 0.0),
    "top-p 0.9": (-1, 0.9, 0.0),
    "all three": (50, 0.9, 0.02),
}
IMPLS = ("kernel", "native", "torch")
CACHE_BYTES = 256 << 20


def _time_alternating(cands, reps, window_s=0.1):
    """{name: (median, min, max) us per call}; fn(i) is call i, and every
    window ends in a device synchronise."""
    import torch

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / iters

    iters = {}
    for name, fn in cands.items():
        window(fn, 3)  # warm-up
        iters[name] = max(3, min(2000, int(window_s * 1e6 / window(fn, 3))))
    out = {name: [] for name in cands}
    for _ in range(reps):
        for name, fn in cands.items():
            out[name].append(window(fn, iters[name]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def _runner(sampler):
    """What sample_params reads of a ModelRunner, without a model."""
    import torch

    from production_stack_amd.engine.model_runner import ModelRunner

    stub = types.SimpleNamespace(
        config=types.SimpleNamespace(sampler=sampler, seed=0),
        _generator=torch.Generator(device="cpu").manual_seed(12345),
        _native_draws=1 << 32,
    )
    for name in ("sample_params", "_sample_records", "_redraw_seeded"):
        setattr(stub, name, types.MethodType(getattr(ModelRunner, name), stub))
    return stub


def worker(V, reps):
    import torch

    from production_stack_amd import ops
    from production_stack_amd.engine.sampling import SamplingParams

    assert torch.cuda.is_available() and ops.HAVE_EXT
    native, eager = _runner("native"), _runner("torch")
    for R in RS:
        torch.manual_seed(V + R)
        n = max(2, min(8, 2 * CACHE_BYTES // (R * V * 2) + 1))
        logits = [(torch.randn(R, V, device="cuda") * 4).to(torch.bfloat16)
                  for _ in range(n)]
        for fname, (top_k, top_p, min_p) in FILTERS.items():
            params = [SamplingParams(temperature=0.8, top_k=top_k,
                                     top_p=top_p, min_p=min_p)] * R
            rec = native._sample_records(None, params).cuda()
            cands = {
                "kernel": lambda i: ops.sample(logits[i % n], rec),
                "native": lambda i: native.sample_params(
                    logits[i % n], params),
                "torch": lambda i: eager.sample_params(logits[i % n], params),
            }
            cell = {"V": V, "R": R, "filters": fname, "copies": n}
            for k, (med, lo, hi) in _time_alternating(cands, reps).items():
                cell[k + "_us"] = round(med, 1)
                cell[k + "_min_us"] = round(lo, 1)
                cell[k + "_max_us"] = round(hi, 1)
            print("CELL " + json.dumps(cell), flush=True)
        del logits
        torch.cuda.empty_cache()


def _markdown(cells):
    out = ["| V | R | filters | kernel us (min..max) | native us (min..max) "
           "| torch us (min..max) | torch / native |",
           "|---|---|---|---|---|---|---|"]
    for c in cells:
        out.append(
            f"| {c['V']} | {c['R']} | {c['filters']} | "
            + " | ".join(
                f"{c[k + '_us']} ({c[k + '_min_us']}..{c[k + '_max_us']})"
                for k in IMPLS)
            + f" | {c['torch_us'] / c['native_us']:.1f}x |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vs", type=int, nargs="*", default=list(VS))
    ap.add_argument("--reps", type=int, default=3,
                    help="rounds of alternating timed windows")
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed to each child process")
    ap.add_argument("--md", default=None,
                    help="write the table to this markdown file")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--v", type=int)
    a = ap.parse_args()
    if a.worker:
        worker(a.v, a.reps)
        return
    cells = []
    for V in a.vs:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable,
               os.path.abspath(__file__), "--worker", "--v", str(V),
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(f"V={V} ended with status {r.returncode}; stopping",
                  flush=True)
            sys.exit(1)
        cells += [json.loads(line[5:]) for line in r.stdout.splitlines()
                  if line.startswith("CELL ")]
    if a.md:
        with open(a.md, "w") as f:
            f.write(_markdown(cells))


if __name__ == "__main__":
    main()
