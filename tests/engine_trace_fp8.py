"""Launch trace of VitEngine(dtype="mxfp8", fp8_attn=True): engine_trace.py's recorder (through engine_trace_ln.record: its _patch,
names and torch-op mode) on the classifier whose qkv product stays an MXFP8 operand (linear_mxfp8_q into qkv8 / qkv8s) and whose
attention is attention_fp8; test_attn_fp8_cpu.py is its test.

The fixture tests/golden/engine_trace_fp8.json is written by `python tests/engine_trace_fp8.py --write`."""
from __future__ import annotations

import os
import sys

import pytest

import engine_trace as et
import engine_trace_ln as etl
import trainer_trace as tt

FIXTURE = os.path.join(tt.HERE, "golden", "engine_trace_fp8.json")
VAR = "YV_VIT_FP8_ATTN"
P16, P8 = "vit_tiny_test", "vit_tiny8_test"              # two blocks, 197 and 785 tokens
# case -> (model, constructor arguments, environment, device count)
CASES = {
    "vit_tiny_mxfp8_fp8_attn": (P16, dict(dtype="mxfp8", fp8_attn=True), {}, False),
    "vit_tiny_mxfp8_fp8_attn_mid": (P16, dict(dtype="mxfp8", fp8_attn=True, mid_gemm=True), {}, True),
    "vit_tiny8_mxfp8_fp8_attn": (P8, dict(dtype="mxfp8", fp8_attn=True, long_attn=True), {}, True),
    "vit_tiny8_mxfp8_fp8_attn_mid_env": (P8, dict(dtype="mxfp8", mid_gemm=True), {VAR: "1"}, False),
}


def record(name: str, kw: dict, env: dict, with_count: bool = False) -> list:
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv(VAR, raising=False)
        return etl.record(name, kw, env, with_count)


def record_case(case: str) -> list:
    return record(*CASES[case])


def load_fixture() -> dict:
    return et.json.load(open(FIXTURE, encoding="utf-8"))


if __name__ == "__main__":
    root = os.path.dirname(tt.HERE)
    sys.path[:0] = [root, os.path.join(root, "yolov8-vit_amd")]
    text = et.dumps({case: record_case(case) for case in CASES})
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"wrote {FIXTURE}: {len(text)} bytes, {text.count(chr(10))} lines")
    else:
        sys.stdout.write(text)
