"""Step-boundary idle time from a rocprofv3 kernel trace.

Usage:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python bench.py --gpus 1 --steps 64 --warmup 48
    python csrc/tools/step_gap_stats.py DIR [--steps 64]

`greedy_sample_kernel` ends a forward. For each of the last --steps forwards
the tool prints the gap between the end of the previous forward's sampling
kernel and the start of the forward's first kernel (the step-boundary gap:
what the host spends before it launches the step), the sum of all other
inter-kernel gaps inside the forward, and the kernel time per forward by
group over the whole trace, in the form of the tables in profiles/README.md.
"""

import argparse
import csv
import glob
import json
import os
import statistics
import sys

GROUPS = (
    ("paged_attn_decode_kernel", ("paged_attn_decode_kernel",)),
    ("gemm", ("Cijk_", "gemm8p", "skinny_gemm")),
    ("prefill_attention_combines_order",
     ("paged_attn_prefill", "combine", "decode_order")),
)


def group_of(name: str) -> str:
    for group, keys in GROUPS:
        if any(k in name for k in keys):
            return group
    return "everything_else"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    paths = glob.glob(
        os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True
    )
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {args.dir}")
    rows = []
    for path in paths:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]),
                             int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    ends = [i for i, r in enumerate(rows) if "greedy_sample_kernel" in r[2]]
    if len(ends) < args.steps + 1:
        sys.exit(f"only {len(ends)} forwards in the trace")

    per_group = {}
    for s, e, name in rows:
        g = group_of(name)
        per_group[g] = per_group.get(g, 0) + (e - s)
    forwards = len(ends)

    boundary, inner, busy, span = [], [], [], []
    largest, largest_at = [], []
    for k in range(len(ends) - args.steps, len(ends)):
        first, last = ends[k - 1] + 1, ends[k]
        boundary.append(rows[first][0] - rows[first - 1][1])
        gaps = 0
        big, big_at = 0, 0
        horizon = rows[first][1]
        for i in range(first + 1, last + 1):
            g = max(0, rows[i][0] - horizon)
            gaps += g
            if g > big:
                big, big_at = g, i - first
            horizon = max(horizon, rows[i][1])
        inner.append(gaps)
        largest.append(big)
        largest_at.append(big_at)
        busy.append(sum(rows[i][1] - rows[i][0]
                        for i in range(first, last + 1)))
        span.append(rows[last][1] - rows[first - 1][1])

    def ms(v):
        return round(v / 1e6, 3)

    q = statistics.quantiles(boundary, n=10)
    print(json.dumps({
        "forwards_in_trace": forwards,
        "timed_steps": args.steps,
        "boundary_gap_ms": {
            "median": ms(statistics.median(boundary)),
            "p10": ms(q[0]), "p90": ms(q[-1]),
            "min": ms(min(boundary)), "max": ms(max(boundary)),
        },
        "other_gaps_ms_median": ms(statistics.median(inner)),
        # the largest single gap inside a forward and the index of the
        # kernel it precedes (a host sync before the layer stack shows here)
        "largest_inner_gap_ms_median": ms(statistics.median(largest)),
        "largest_inner_gap_before_kernel_median": statistics.median(
            largest_at),
        "kernels_per_timed_forward_median": statistics.median(
            ends[k] - ends[k - 1]
            for k in range(len(ends) - args.steps, len(ends))),
        "kernel_ms_per_timed_forward_median": ms(statistics.median(busy)),
        "sample_end_to_sample_end_ms_median": ms(statistics.median(span)),
        "kernel_ms_per_forward_whole_trace": {
            g: round(v / 1e6 / forwards, 3)
            for g, v in sorted(per_group.items())
        },
        "kernel_ms_per_forward_total": round(
            sum(per_group.values()) / 1e6 / forwards, 3),
    }, indent=1))


if __name__ == "__main__":
    main()
