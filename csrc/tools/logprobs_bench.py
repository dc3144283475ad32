#!/usr/bin/env python3
"""Logprobs probe: ops.logprobs (csrc/logprobs.hip) against the torch path.

At V = 128256, for R in {1, 16, 256} with every row asking and N in {0, 5, 20}
alternatives, and for the prompt case (2048 rows, N = 0), it times
  kernel  ops.logprobs alone: token ids already on the device, back-to-back
          launches
  native  what ModelRunner.sample adds under sampler="native": one launch and
          the copy of the three small outputs to the host
  torch   what it ran before: index_select / float / log_softmax / gather /
          .cpu(), then per row a topk and two more .cpu() calls; for the
          prompt case log_softmax(logits.float()), a gather and one .cpu()
native and torch end in a device-to-host copy, so every window is timed with
a host clock around calls that end in a device synchronise; the candidates
alternate within each of the --reps rounds, one window each, a window sized
to about 0.1 s from a calibration call (3 calls at least). Each call reads
the next of several logits copies (up to 8, together above the 256 MiB
Infinity Cache where 8 suffice). It prints the median us with the min..max
spread; --md FILE writes the table as markdown.

The driver starts one child process per R, each under its own time limit, and
stops at the first one that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

V = 128256
CASES = {1: (0, 5, 20), 16: (0, 5, 20), 256: (0, 5, 20), 2048: (0,)}
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


def torch_sampled(logits, sampled, n_top):
    """ModelRunner.sample's logprobs block before ops.logprobs, every row
    asking; `sampled` is the host tensor sample_params returns."""
    import torch

    want = list(range(logits.shape[0]))
    idx = torch.tensor(want, dtype=torch.long, device=logits.device)
    lp = torch.log_softmax(logits.index_select(0, idx).float(), dim=-1)
    chosen = sampled[idx.cpu()].to(lp.device)
    vals = lp.gather(1, chosen.unsqueeze(1)).squeeze(1).cpu()
    out = []
    for j in want:
        top = None
        if n_top > 0:
            tv, ti = lp[j].topk(n_top)
            top = list(zip((int(t) for t in ti.cpu()),
                           (float(v) for v in tv.cpu())))
        out.append((float(vals[j]), top))
    return out


def torch_prompt(logits, ids):
    """_collect_prompt_logprobs before ops.logprobs, for one chunk."""
    import torch

    lg = torch.log_softmax(logits.float(), dim=-1)
    return [float(v) for v in lg.gather(1, ids.unsqueeze(1)).squeeze(1).cpu()]


def worker(R, reps):
    import torch

    from production_stack_amd import ops

    assert torch.cuda.is_available() and ops.HAVE_EXT
    torch.manual_seed(R)
    n = max(2, min(8, 2 * CACHE_BYTES // (R * V * 2) + 1))
    logits = [(torch.randn(R, V, device="cuda") * 4).to(torch.bfloat16)
              for _ in range(n)]
    ids = torch.randint(0, V, (R,), device="cuda")
    ids_host = ids.cpu()
    for N in CASES[R]:
        def native(i):
            return [t.cpu() for t in ops.logprobs(logits[i % n], ids, N)]

        if R == 2048:
            def eager(i):
                return torch_prompt(logits[i % n], ids)
        else:
            def eager(i):
                return torch_sampled(logits[i % n], ids_host, N)

        cands = {
            "kernel": lambda i: ops.logprobs(logits[i % n], ids, N),
            "native": native,
            "torch": eager,
        }
        cell = {"V": V, "R": R, "N": N, "copies": n}
        for k, (med, lo, hi) in _time_alternating(cands, reps).items():
            cell[k + "_us"] = round(med, 1)
            cell[k + "_min_us"] = round(lo, 1)
            cell[k + "_max_us"] = round(hi, 1)
        print("CELL " + json.dumps(cell), flush=True)


def _markdown(cells):
    out = ["| V | R | N | kernel us (min..max) | native us (min..max) "
           "| torch us (min..max) | torch / native |",
           "|---|---|---|---|---|---|---|"]
    for c in cells:
        out.append(
            f"| {c['V']} | {c['R']} | {c['N']} | "
            + " | ".join(
                f"{c[k + '_us']} ({c[k + '_min_us']}..{c[k + '_max_us']})"
                for k in IMPLS)
            + f" | {c['torch_us'] / c['native_us']:.1f}x |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rs", type=int, nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=5,
                    help="rounds of alternating timed windows")
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed to each child process")
    ap.add_argument("--md", default=None,
                    help="write the table to this markdown file")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--r", type=int)
    a = ap.parse_args()
    if a.worker:
        worker(a.r, a.reps)
        return
    cells = []
    for R in a.rs:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable,
               os.path.abspath(__file__), "--worker", "--r", str(R),
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(f"R={R} ended with status {r.returncode}; stopping",
                  flush=True)
            sys.exit(1)
        cells += [json.loads(line[5:]) for line in r.stdout.splitlines()
                  if line.startswith("CELL ")]
    if a.md:
        with open(a.md, "w") as f:
            f.write(_markdown(cells))


if __name__ == "__main__":
    main()
