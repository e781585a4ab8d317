"""Launch trace of YoloEngine(grouped_head=True): engine_trace.py's recorder (its _patch, names and torch-op mode) on the engine
with the grouped Detect head; test_engine_trace_grouped_cpu.py is its test.

A conv2d_group line holds its members as conv2d's argument lists, (in0, in1, B, Hout, Wout, ksize, stride, weight, bias, out,
out_c_off, flags, res, res_c_off); `expand` writes each member as the conv2d line the ungrouped engine records for it.

The fixture tests/golden/engine_trace_grouped.json is written by `python tests/engine_trace_grouped.py --write`."""
from __future__ import annotations

import json
import os
import sys

import pytest
import torch

import engine_trace as et
import trainer_trace as tt

FIXTURE = os.path.join(tt.HERE, "golden", "engine_trace_grouped.json")
# case -> (constructor arguments, the case of engine_trace.json it regroups)
CASES = {
    "yolo_n5_bf16_grouped": (dict(scale="n", nc=5, dtype="bf16"), "yolo_n5_bf16"),
    "yolo_n5_mxfp8_grouped": (dict(scale="n", nc=5, dtype="mxfp8"), "yolo_n5_mxfp8"),
}


def record_case(case: str) -> list:
    from yvhip import engines
    kw, _ = CASES[case]
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        et._patch(mp, rec)
        eng = engines.YoloEngine(engines.init_yolo_state(kw["scale"], kw["nc"]), size=et.SIZE, device="cpu", grouped_head=True, **kw)
        images = torch.zeros((et.B, et.SIZE, et.SIZE, 3), dtype=torch.uint8)
        rec.walk("images", images)
        et._yolo_names(rec, eng, eng._buffers(et.B))
        rec.recording = True
        with tt._TorchOps(rec):
            eng(images)
        rec.recording = False
    return json.loads(json.dumps(rec.trace))


def expand(calls: list) -> list:
    """Every conv2d_group line replaced by one conv2d line per member, as native_stub spells a conv2d call: the twelve parameters
    without a default, then res / res_c_off by name where they are not the defaults."""
    out = []
    for c in calls:
        if c[0] != "conv2d_group":
            out.append(c)
            continue
        for m in c[2][0]:
            line = ["conv2d", c[1], m[:12]]
            kw = {k: v for k, v, d in (("res", m[12], None), ("res_c_off", m[13], 0)) if v != d}
            out.append(line + [kw] if kw else line)
    return out


def load_fixture() -> dict:
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


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
