#!/usr/bin/env python3
"""MoE expert-MLP probe: per-expert loop (hipBLASLt) vs csrc/moe_fused.hip.

Layer table: one Mixtral-8x7B-shaped MoE MLP (E=8, H=4096, I=14336,
top_k=2) at decode batch sizes T; routing included on both sides since the
layer computes it either way. Windows alternate between the paths and the
median window is reported. The fused path's effective weight bandwidth is
(bytes of the experts that received a token) / (time of the fused op alone).

--engine adds mini-mixtral decode steps/s with moe_backend=loop,
fused + enforce_eager and fused + hipGraphs (kernel effect vs capture).
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(
    0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
)
import torch  # noqa: E402

from production_stack_amd import ops  # noqa: E402
from production_stack_amd.engine.config import (  # noqa: E402
    ARCHITECTURES,
    CacheConfig,
    EngineConfig,
    SchedulerConfig,
)


def _window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_layer(Ts, iters, windows):
    from production_stack_amd.engine.models.llama import LlamaLayer

    cfg = dataclasses.replace(ARCHITECTURES["mixtral-8x7b"], num_layers=1)
    torch.manual_seed(0)
    with torch.device("cuda"):
        layer = LlamaLayer(cfg, tp=1)
    with torch.no_grad():
        for p in layer.parameters():
            p.normal_(0, 0.02)
        layer.moe_gate.normal_(0, 1.0)
    E, H, I, K = cfg.num_experts, cfg.hidden_size, layer.inter, layer.top_k
    expert_bytes = 3 * H * I * 2
    print(f"layer: E={E} H={H} I={I} top_k={K}  "
          f"({expert_bytes / 1e6:.0f} MB per expert)")
    print("   T  experts   loop us  fused us  graph us  op us   op GB/s")
    for T in Ts:
        x = torch.randn(T, H, device="cuda").to(torch.bfloat16)

        def run(backend):
            layer.moe_backend = backend
            with torch.no_grad():
                return layer._moe_forward(x)

        # routing of this x, for the byte count and the op-only timing
        with torch.no_grad():
            probs = torch.softmax(
                torch.nn.functional.linear(x.float(), layer.moe_gate.float()),
                dim=-1,
            )
            w, sel = torch.topk(probs, K, dim=-1)
            w = w / w.sum(dim=-1, keepdim=True)
        active = int(sel.unique().numel())

        def op():
            return ops.fused_moe(
                x, layer.experts_gate_up, layer.experts_down, sel, w
            )

        diff = (run("fused").float() - run("loop").float()).abs().max().item()
        for _ in range(10):  # warm every path and shape
            run("loop"), run("fused"), op()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run("fused")
        graph.replay()
        t = {"loop": [], "fused": [], "graph": [], "op": []}
        for _ in range(windows):
            t["loop"].append(_window(lambda: run("loop"), iters))
            t["fused"].append(_window(lambda: run("fused"), iters))
            t["graph"].append(_window(graph.replay, iters))
            t["op"].append(_window(op, iters))
        m = {k: statistics.median(v) for k, v in t.items()}
        gbs = active * expert_bytes / m["op"] / 1e9
        print(f"{T:4d}  {active:7d}  {m['loop'] * 1e6:8.1f}  "
              f"{m['fused'] * 1e6:8.1f}  {m['graph'] * 1e6:8.1f}  "
              f"{m['op'] * 1e6:6.1f}  {gbs:8.0f}   "
              f"(max |fused-loop| {diff:.4f})")


def bench_engine(batch, steps):
    from production_stack_amd.engine.engine import LLMEngine
    from production_stack_amd.engine.sampling import SamplingParams

    print(f"mini-mixtral decode, batch {batch}, {steps} steps:")
    for name, kw in (
        ("loop", dict(moe_backend="loop")),
        ("fused+eager", dict(moe_backend="fused", enforce_eager=True)),
        ("fused+graphs", dict(moe_backend="fused")),
    ):
        cfg = EngineConfig(
            model="mini-mixtral",
            max_model_len=1024,
            cache=CacheConfig(num_gpu_blocks=512, block_size=16),
            scheduler=SchedulerConfig(
                max_num_seqs=batch, max_num_batched_tokens=2048
            ),
            **kw,
        )
        eng = LLMEngine(cfg, device="cuda")
        p = SamplingParams(
            max_tokens=steps + 8, temperature=0.0, ignore_eos=True
        )
        for rep in range(2):  # first pass warms, second is reported
            for i in range(batch):
                eng.add_request(
                    f"r{rep}-{i}", list(range(10 + i, 74 + i)), p
                )
            times = []
            while eng.has_unfinished():
                t0 = time.perf_counter()
                eng.step()
                times.append(time.perf_counter() - t0)
        dec = times[4:-1]  # drop prefill / ramp steps and the final one
        med = statistics.median(dec)
        print(f"  {name:13s} graphs={eng.runner.graphs is not None!s:5s} "
              f"{1.0 / med:8.1f} steps/s  ({med * 1e6:.0f} us/step median "
              f"of {len(dec)})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--engine-batch", type=int, default=8)
    ap.add_argument("--engine-steps", type=int, default=128)
    ap.add_argument("--skip-layer", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_bench needs a GPU"
    if not args.skip_layer:
        bench_layer(args.T, args.iters, args.windows)
    if args.engine:
        bench_engine(args.engine_batch, args.engine_steps)
