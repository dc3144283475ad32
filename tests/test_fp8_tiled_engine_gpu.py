"""mini-llama served with quantization="fp8", fp8_gemm="native_tiled": a
300-token prefill step runs csrc/gemm_fp8_tiled.hip for every dense
projection, the decode steps after it csrc/skinny_gemm_fp8.hip."""

import dataclasses

import pytest

from production_stack_amd import ops
from production_stack_amd.engine.engine import LLMEngine
from tests.test_fp8_native_engine_gpu import PARAMS, _config

pytestmark = pytest.mark.gpu

PROMPT = [50 + i % 200 for i in range(300)]


def test_prefill_tiled_decode_skinny(monkeypatch):
    # _config pins fp8_gemm="native" itself
    cfg = dataclasses.replace(_config(enforce_eager=True),
                              fp8_gemm="native_tiled")
    eng = LLMEngine(cfg, device="cuda")
    layers = len(eng.runner.model.layers)
    calls = {"skinny_gemm_fp8": [], "gemm_fp8_tiled": []}
    real = {name: getattr(ops, name) for name in calls}
    for name in calls:
        def shim(*a, _name=name):
            calls[_name].append(a[0].shape[0])
            return real[_name](*a)

        monkeypatch.setattr(ops, name, shim)

    eng.add_request("r", PROMPT, PARAMS)
    out, per_step = [], []
    while eng.has_unfinished():
        for c in calls.values():
            del c[:]
        for o in eng.step():
            out.extend(o.new_token_ids)
        per_step.append({k: list(v) for k, v in calls.items()})
    assert len(out) == 8
    assert per_step[0] == {"skinny_gemm_fp8": [],
                           "gemm_fp8_tiled": [300] * (4 * layers)}, per_step
    assert len(per_step) == 8  # the prefill step samples token 0
    for c in per_step[1:]:
        assert c == {"skinny_gemm_fp8": [1] * (4 * layers),
                     "gemm_fp8_tiled": []}, per_step
