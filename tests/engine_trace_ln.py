"""Launch trace of VitEngine(ln_gemm=True): engine_trace.py's recorder (its _patch, names and torch-op mode) on the classifier whose
norm1 -> qkv and norm2 -> fc1 steps are linear_ln calls; test_engine_trace_ln_cpu.py is its test.

A linear_ln line holds (x, gamma, beta, h, w, bias, out) and, by name, what differs from the defaults (flags, m_dev, m_mul);
`expand` writes it as the layernorm + linear pair the engine without the flag records for the same step.  get_option answers with
the value last set, so the pass runs between set_option("linear_ln_mid", MID_GEMM_ROWS) and its restore, as on the device.

The fixture tests/golden/engine_trace_ln.json is written by `python tests/engine_trace_ln.py --write`."""
from __future__ import annotations

import json
import os
import sys

import pytest
import torch

import engine_trace as et
import trainer_trace as tt

FIXTURE = os.path.join(tt.HERE, "golden", "engine_trace_ln.json")
ENV_VARS = ("YV_VIT_FUSED_LN", "YV_VIT_LONG_ATTN", "YV_MX_ATTN_FUSED", "YV_VIT_MID_GEMM", "YV_VIT_LN_GEMM")
# case -> (model, constructor arguments, environment, device count, the case of engine_trace.json it is compared with)
CASES = {
    "vit_bf16_full_ln_gemm": (et.P16, dict(cls_tail=False, ln_gemm=True), {}, False, "vit_bf16_full"),
    "vit_bf16_tail_ln_gemm": (et.P16, dict(cls_tail=True, ln_gemm=True), {}, False, "vit_bf16_tail"),
    "vit_bf16_count_ln_gemm": (et.P16, dict(ln_gemm=True), {}, True, "vit_bf16_count"),
    "vit_bf16_tail_ln_gemm_env": (et.P16, dict(cls_tail=True), {"YV_VIT_LN_GEMM": "1"}, False, "vit_bf16_tail"),
    "vit_p8_bf16_long_ln_gemm": (et.P8, dict(long_attn=True, ln_gemm=True), {}, False, "vit_p8_bf16_long"),
}
# the flag unset / ignored: these record the named case of engine_trace.json unchanged
UNCHANGED = {
    "unset": (et.P16, dict(cls_tail=False, fused_ln=False), {}, "vit_bf16_full"),
    "env_with_fused_ln": (et.P16, dict(cls_tail=True, fused_ln=True), {"YV_VIT_LN_GEMM": "1"}, "vit_bf16_tail_ln"),
    "env_with_mxfp8": (et.P16, dict(dtype="mxfp8"), {"YV_VIT_LN_GEMM": "1"}, "vit_mxfp8"),
}


def build(mp, name: str, kw: dict, env: dict):
    """A CPU VitEngine of one of trainer_trace's three-block models under `env` (call inside et._patch)."""
    from yvhip import engines
    for var in ENV_VARS:
        mp.delenv(var, raising=False)
    for var, value in env.items():
        mp.setenv(var, value)
    for model, cfg in tt.MODELS.items():
        mp.setitem(engines.VIT_CFGS, model, cfg)
    return engines.VitEngine(engines.init_vit_wrapper_state(name, et.NUM_CLASSES, seed=2), name, et.NUM_CLASSES, device="cpu", **kw)


def record(name: str, kw: dict, env: dict, with_count: bool = False) -> list:
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        et._patch(mp, rec)
        eng = build(mp, name, kw, env)
        for attr in ("w_pe", "b_pe", "cls", "pos", "blocks", "nw", "nb", "w_head", "b_head", "fc1w", "fc1b", "fc2w", "fc2b"):
            rec.walk(attr, getattr(eng, attr))
        patches = eng.patch_buffer(et.CAP)
        rec.walk("", eng._buffers(et.CAP))
        io = dict(logits=torch.zeros(et.CAP, et.NUM_CLASSES), labels=torch.zeros(et.CAP, dtype=torch.int32),
                  count=torch.full((1,), et.CAP - 1, dtype=torch.int32) if with_count else None)
        rec.walk("", io)
        rec.recording = True
        with tt._TorchOps(rec), eng.guard(0):
            feats = eng.backbone(patches, et.CAP, io["count"], 0)
            eng.head(feats, et.CAP, io["logits"], io["labels"], count=io["count"])
        rec.recording = False
    return json.loads(json.dumps(rec.trace))


def record_case(case: str) -> list:
    name, kw, env, with_count, _ = CASES[case]
    return record(name, kw, env, with_count)


def expand(calls: list, D: int) -> list:
    """Every linear_ln line replaced by the layernorm and the linear line of the pair it stands for, as native_stub spells them."""
    out = []
    for c in calls:
        if c[0] != "linear_ln":
            out.append(c)
            continue
        x, gamma, beta, h, w, bias, dst = c[2]
        kw = c[3] if len(c) > 3 else {}
        assert set(kw) <= {"flags", "m_dev", "m_mul"}, kw
        n = kw.get("m_mul", 1)
        ln_kw = {k: v for k, v in (("count_dev", kw.get("m_dev")), ("rows_per_count", n)) if v is not None}
        out.append(["layernorm", c[1], [x, gamma, beta, h, et.CAP * n, D, D, D], ln_kw])
        out.append(["linear", c[1], [h, w, bias, dst], kw])
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
