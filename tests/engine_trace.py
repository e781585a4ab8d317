"""Launch-trace recorder of YoloEngine and VitEngine (a helper module like trainer_trace.py, whose Recorder, stream fakes, torch-op
mode and wrapper stub it uses; test_engine_trace_cpu.py is its test).

`record_case` builds an engine on the CPU, runs one replay of its launch list with nothing launched and returns, in order, what
the engine would have put on the stream:
  * every native wrapper that yvhip.engines imports (each function of the yvhip package among the module's globals, bar the
    host-only require_gpu and mx_map) is a recording stub; set_option / get_option are recorded too (get_option answers with
    the value last set); the quantisers answer with a (q, scales) pair, detect_tail / detect_decode with (boxes, scores);
  * view / mx_view build operands and launch nothing: their stubs add no line, the operand shows inside the call that consumes it
    as [tensor, channel offset, channels, up] (an MX view names the map's byte tensor);
  * torch's own kernels (mutating aten ops, clone, _to_copy) are lines as well.
Detector cases: init_yolo_state(scale, nc), SIZE x SIZE images, batch B, one __call__ (or a bare forward_raw); "flip" cases run
one replay unrecorded, set fused_c2f = False on the same engine and record the next.  Classifier cases: the three-block models
of trainer_trace.MODELS, CAP crops, backbone + head under the slot's guard.

Tensor operands are written by name (trainer_trace's notation).  The detector's weights are "w." / "b." / "wq." + state-dict key
(plus the engine's derived det{s}.0, .pad and .pad16 entries), its buffers out{idx} / y{idx} / t{idx} / det{s}.{hb,hc,box,cls}
and "mx." + buffer + ".0" (bytes) / ".1" (scales); the classifier's are the engine's own attributes and buffer keys.  The names
do not depend on how the engine files its buffers.  A case holds its calls only: shapes are pinned by the views and sizes in them.

The fixture tests/golden/engine_trace.json is written by `python tests/engine_trace.py --write`, one line per call."""
from __future__ import annotations

import collections
import inspect
import json
import os
import sys

import pytest
import torch

import trainer_trace as tt

FIXTURE = os.path.join(tt.HERE, "golden", "engine_trace.json")
HOST_ONLY = ("require_gpu", "mx_map")                   # functions of the package that launch nothing
B, SIZE, CAP, NUM_CLASSES = 2, 64, 3, 5
View = collections.namedtuple("View", "t c_off c up")

YOLO_CASES = {
    "yolo_n5_bf16": dict(scale="n", nc=5, dtype="bf16"),                       # fused C2f blocks, fused tail
    "yolo_n5_bf16_unfused": dict(scale="n", nc=5, dtype="bf16", flip=True),
    "yolo_n80_bf16": dict(scale="n", nc=80, dtype="bf16"),                     # detect_decode: no fused tail
    "yolo_n5_mxfp8": dict(scale="n", nc=5, dtype="mxfp8"),
    "yolo_s5_mxfp8": dict(scale="s", nc=5, dtype="mxfp8"),
    "yolo_m5_mxfp8": dict(scale="m", nc=5, dtype="mxfp8"),                     # c = 48 block in bf16, two-source MX cv1
    "yolo_n5_bf16_forward_raw": dict(scale="n", nc=5, dtype="bf16", raw=True),
    "yolo_n5_mxfp8_unfused": dict(scale="n", nc=5, dtype="mxfp8", flip=True),
}
P16, P8 = "vit_tiny3_test", "vit_tiny3p8_test"
VIT_CASES = {
    "vit_bf16_tail_ln": (P16, dict(cls_tail=True, fused_ln=True)),
    "vit_bf16_tail": (P16, dict(cls_tail=True, fused_ln=False)),
    "vit_bf16_full_ln": (P16, dict(cls_tail=False, fused_ln=True)),
    "vit_bf16_full": (P16, dict(cls_tail=False, fused_ln=False)),
    "vit_bf16_full_cus_from_1": (P16, dict(full_cus_from=1)),
    "vit_mxfp8": (P16, dict(dtype="mxfp8")),
    "vit_mxfp8_attn_unfused": (P16, dict(dtype="mxfp8", env={"YV_MX_ATTN_FUSED": "0"})),
    "vit_p8_bf16_long": (P8, dict(long_attn=True)),
    "vit_p8_mxfp8_long": (P8, dict(dtype="mxfp8", long_attn=True)),
    "vit_p8_mxfp8_long_attn_unfused": (P8, dict(dtype="mxfp8", long_attn=True, env={"YV_MX_ATTN_FUSED": "0"})),
    "vit_bf16_count": (P16, dict(count=True)),
}
CASES = list(YOLO_CASES) + list(VIT_CASES)


def _patch(mp, rec):
    from yvhip import engines
    options = {}
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)

    def quantised(given):                              # quant_mxfp8(x, q, scales) / quant_conv_weight_mxfp8(w)
        x = given.get("x", given.get("w"))
        rows, k = x.shape
        q, s = given.get("q"), given.get("scales")
        return (u8(rows, (k + 127) // 128 * 128) if q is None else q,
                u8((k + 127) // 128, (rows + 255) // 256 * 256, 4) if s is None else s)

    def detections(given):                             # detect_tail(feats, ...) / detect_decode(box_logits, ...)
        n = given.get("feats", given.get("box_logits"))[0].shape[0]
        return torch.zeros(n, 1, 4), torch.zeros(n, 1, given["nc"])

    results = {"quant_mxfp8": quantised, "quant_conv_weight_mxfp8": quantised, "detect_tail": detections,
               "detect_decode": detections, "quant_mxfp8_map": lambda given: given["out"],
               "set_option": lambda given: options.__setitem__(given["key"], given["value"]),
               "get_option": lambda given: options.get(given["key"], 1)}
    natives = {n: v for n, v in vars(engines).items()
               if inspect.isfunction(v) and v.__module__ == "yvhip" and n not in HOST_ONLY}
    assert set(results) | {"view", "mx_view", "conv2d", "conv2d_mxfp8", "c2f_fused", "attention_long", "wrapper_head"} \
        <= set(natives), sorted(natives)
    for n, real in natives.items():
        mp.setattr(engines, n, tt.native_stub(rec, n, real, results.get(n, lambda given: None)))
    mp.setattr(engines, "view", lambda t, c_off, c, up=0: View(t, c_off, c, up))
    mp.setattr(engines, "mx_view", lambda m, c_off, c, up=0: View(m[0], c_off, c, up))
    mp.setattr(engines, "require_gpu", lambda: None)
    mp.setattr(torch.cuda, "synchronize", lambda device=None: None)
    mp.setattr(torch.cuda, "current_stream", lambda device=None: rec.stack[-1])


def _yolo_names(rec, eng, bufs):
    """Names that hold however the engine files its buffers: by layer and kind, flat by name, or both."""
    rec.walk("w", eng.w)
    rec.walk("b", eng.b)
    rec.walk("wq", eng.wq)
    for k, v in bufs.items():
        if k in ("out", "y", "t"):
            for idx, t in v.items():
                rec.walk(f"{k}{idx}", t)
        elif k == "mx":
            rec.walk("mx", v)
        elif isinstance(v, torch.Tensor):
            rec.walk(k, v)
        elif k == "flat":
            rec.walk("", v)


def _record_yolo(rec, case):
    from yvhip import engines
    kw = dict(YOLO_CASES[case])
    flip, raw = kw.pop("flip", False), kw.pop("raw", False)
    eng = engines.YoloEngine(engines.init_yolo_state(kw["scale"], kw["nc"]), size=SIZE, device="cpu", **kw)
    images = torch.zeros((B, SIZE, SIZE, 3), dtype=torch.uint8)
    rec.walk("images", images)
    _yolo_names(rec, eng, eng._buffers(B))
    if flip:
        eng(images)
        eng.fused_c2f = False
    rec.recording = True
    with tt._TorchOps(rec):
        eng.forward_raw(images) if raw else eng(images)
    rec.recording = False


def _record_vit(rec, case, mp):
    from yvhip import engines
    name, kw = VIT_CASES[case]
    kw = dict(kw)
    env, full_cus_from, with_count = kw.pop("env", {}), kw.pop("full_cus_from", None), kw.pop("count", False)
    for var in ("YV_VIT_FUSED_LN", "YV_VIT_LONG_ATTN", "YV_MX_ATTN_FUSED"):
        mp.delenv(var, raising=False)
    for var, value in env.items():
        mp.setenv(var, value)
    for model, cfg in tt.MODELS.items():
        mp.setitem(engines.VIT_CFGS, model, cfg)
    eng = engines.VitEngine(engines.init_vit_wrapper_state(name, NUM_CLASSES, seed=2), name, NUM_CLASSES, device="cpu", **kw)
    eng.full_cus_from = full_cus_from
    for attr in ("w_pe", "b_pe", "cls", "pos", "blocks", "nw", "nb", "w_head", "b_head", "fc1w", "fc1b", "fc2w", "fc2b"):
        rec.walk(attr, getattr(eng, attr))
    patches = eng.patch_buffer(CAP)
    rec.walk("", eng._buffers(CAP))
    io = dict(logits=torch.zeros(CAP, NUM_CLASSES), labels=torch.zeros(CAP, dtype=torch.int32),
              count=torch.full((1,), CAP - 1, dtype=torch.int32) if with_count else None)
    rec.walk("", io)
    rec.recording = True
    with tt._TorchOps(rec), eng.guard(0):
        feats = eng.backbone(patches, CAP, io["count"], 0)
        eng.head(feats, CAP, io["logits"], io["labels"], count=io["count"])
    rec.recording = False


def record_case(case: str) -> list:
    """The calls of the case, each [name, stream, positional arguments(, keyword arguments)]."""
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        _patch(mp, rec)
        if case in YOLO_CASES:
            _record_yolo(rec, case)
        else:
            _record_vit(rec, case, mp)
    return json.loads(json.dumps(rec.trace))


def dumps(cases: dict) -> str:
    """The fixture's text: one line per call."""
    line = lambda v: json.dumps(v, separators=(",", ":"))
    return "{\n" + ",\n".join(f"{line(case)}:[\n" + ",\n".join(line(c) for c in calls) + "\n]"
                             for case, calls in cases.items()) + "\n}\n"


def load_fixture() -> dict:
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


if __name__ == "__main__":
    root = os.path.dirname(tt.HERE)
    sys.path[:0] = [root, os.path.join(root, "yolov8-vit_amd")]
    text = dumps({case: record_case(case) for case in CASES})
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"wrote {FIXTURE}: {len(text)} bytes, {text.count(chr(10))} lines")
    else:
        sys.stdout.write(text)
