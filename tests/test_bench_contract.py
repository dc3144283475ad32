"""bench.py driver-contract tests: single-process and torchrun multi-rank
(gloo, CPU) must emit exactly one valid JSON line from rank 0."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(__file__), "..")

COMMON = [
    "--device", "cpu", "--model", "tiny-llama", "--users", "2",
    "--steps", "8", "--warmup", "2", "--max-model-len", "1600",
    "--max-num-batched-tokens", "256",
]


def test_bench_single_process():
    r = subprocess.run(
        [sys.executable, "bench.py"] + COMMON,
        cwd=ROOT, capture_output=True, timeout=420, text=True,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == "output_tokens_per_sec"
    assert out["n_gpus"] == 1
    assert out["value"] > 0
    assert out["steps"] == 8 and out["warmup"] == 2
    assert out["dtype"] == "bfloat16" and out["data"] == "synthetic"
    assert out["higher_is_better"] is True and out["scaling"] == "weak"
    assert "ms_per_step" in out and "config" in out


def _run(extra):
    r = subprocess.run(
        [sys.executable, "bench.py"] + COMMON + extra,
        cwd=ROOT, capture_output=True, timeout=420, text=True,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    import numpy as np

    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_bench_dump_outputs_repeatable(tmp_path):
    """Same arguments, same inputs: two plain runs dump identical float64
    arrays of what the last timed step returned."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _run(["--dump-outputs", a])
    _run(["--dump-outputs", b])
    assert out["steady_state"] == "seeded"
    assert out["ms_per_step"] > 0
    da, db = _load(a), _load(b)
    assert "new_token_ids.npy" in da and list(da) == list(db)
    for name, arr in da.items():
        assert arr.dtype.name == "float64", name
        assert (arr == db[name]).all() and arr.shape == db[name].shape, name
    assert da["new_token_ids.npy"].size == da["num_new_tokens.npy"].sum() > 0
    assert sum(v.nbytes for v in da.values()) <= 64 << 20


def test_bench_full_runs_drained_guard(tmp_path):
    """--full reaches the steady state by real prefill + mixing and keeps
    the same result line and dump format."""
    out = _run(["--full", "--dump-outputs", str(tmp_path)])
    assert out["steady_state"] == "drained"
    assert out["metric"] == "output_tokens_per_sec" and out["value"] > 0
    assert out["steps"] == 8 and out["ms_per_step"] > 0
    assert _load(str(tmp_path))["new_token_ids.npy"].size > 0


@pytest.mark.timeout(400)
def test_bench_torchrun_two_ranks():
    r = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", "29617",
            "bench.py",
        ] + COMMON + ["--gpus", "2"],
        cwd=ROOT, capture_output=True, timeout=380, text=True,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0
