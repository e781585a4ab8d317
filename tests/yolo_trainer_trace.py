"""Launch-trace recorder of YoloTrainer (a helper module like engine_trace.py; trainer_trace.py's Recorder, stream and event fakes,
torch-op mode, wrapper stub and dumps are used as they are; test_yolo_trainer_trace_cpu.py is its test).

`record_case` builds a YoloTrainer on the CPU, runs the case's `step` calls with nothing launched and returns, in order, everything
the trainer would have put on a stream:
  * every native wrapper that yvhip.yolo_training imports (each function of the yvhip package among the module's globals) is a
    recording stub, bar the host-only ones (the workspace sizes and conv_dgrad_s2_route), which run: they decide buffer sizes and
    which blocks take the stride-2 phase data gradient;
  * mview builds an operand and launches nothing: its stand-in adds no line and returns the torch slice of the channels, so that
    the operand shows inside the call that consumes it as name@offset[shape]/[stride] - row pitch, channel window and offset of
    every view are pinned;
  * torch.cuda.current_stream / Stream / Event / stream are trainer_trace's fakes, BucketReducer.reset / ready / finish and torch's
    own kernels (mutating aten ops, clone, _to_copy) are lines as well.
Every case is YOLOv8n, nc 5, 64 x 64 images, batch 2, two boxes per image: all three pyramid levels exist and all five eligible
stride-2 blocks take the phase route where it is asked for.

Tensor operands are written by name (trainer_trace's notation).  The names do not depend on how the trainer files its buffers: the
flat parameter buffers P G Mo P16 RS P_ema RS_ema, z. / dz. / mean. / rstd. + block key, the scratch buffers ws wd_buf col zi xp dzp,
loss_out, the activations x0, out{idx}, y{idx}, t{idx}.{j}, cat{idx}, det{s}.{b0,b1,c0,c1}, the head's det{s}.{box,cls,dbox,dcls},
grad_flat (every activation gradient is a view of it) and the step's images, gt_boxes, gt_labels, gt_counts.

The fixtures tests/golden/yolo_trainer_trace/<case>.json are written by `python tests/yolo_trainer_trace.py --write`, one line per
call."""
from __future__ import annotations

import inspect
import json
import os
import sys

import pytest
import torch

import trainer_trace as tt

FIXTURE_DIR = os.path.join(tt.HERE, "golden", "yolo_trainer_trace")
HOST_ONLY = ("bn_ws_floats", "colsum_ws_floats", "conv_stats_ws_floats", "detect_loss_ws_bytes", "conv_dgrad_s2_route")
SCALE, NC, SIZE, B, GT = "n", 5, 64, 2, 2
FLAGS = ("YV_YOLO_NARROW_WGRAD", "YV_YOLO_FUSED_BN_STATS", "YV_YOLO_PHASE_DGRAD")
CASES = {                                               # case: (steps, constructor arguments)
    "default": (2, dict()),                             # both values of sgd_step's `first`, the side stream and the loss workspace reused
    "all_optins": (1, dict(narrow_wgrad=True, fused_bn_stats=True, phase_dgrad=True)),
    "serial_im2col_adamw_ema": (1, dict(overlap_wgrad=False, implicit_wgrad=False, optimizer="adamw", ema=True)),
}


class _DeviceImages(torch.Tensor):
    """A host tensor that says it is on the device: forward() checks images.is_cuda."""
    is_cuda = property(lambda self: True)


def _patch(mp, rec):
    from yvhip import dist, yolo_training as yt
    natives = {n: v for n, v in vars(yt).items()
               if inspect.isfunction(v) and v.__module__ == "yvhip" and n not in HOST_ONLY + ("mview", "require_gpu")}
    assert {"conv_view", "conv_view_stats", "bn_stats", "bn_stats_finish", "bn_act_fwd", "bn_act_bwd", "conv_dgrad_s2", "view_op",
            "wgrad", "wgrad_conv3", "im2col3", "detect_loss", "sgd_step", "optim_step", "ema_update"} <= set(natives), sorted(natives)
    assert all(inspect.isfunction(getattr(yt, n)) for n in HOST_ONLY)
    for n, real in natives.items():
        mp.setattr(yt, n, tt.native_stub(rec, n, real))
    mp.setattr(yt, "mview", lambda t, c_off=0, c=None: t[..., c_off:t.shape[-1] if c is None else c_off + c])
    mp.setattr(yt, "require_gpu", lambda: None)
    mp.setattr(torch.cuda, "current_stream", lambda device=None: rec.stack[-1])
    mp.setattr(torch.cuda, "Stream", lambda *a, **k: tt._Stream(rec))
    mp.setattr(torch.cuda, "Event", lambda *a, **k: tt._Event(rec))
    mp.setattr(torch.cuda, "stream", lambda s: tt._StreamContext(rec, s))
    for meth in ("reset", "ready", "finish"):
        def traced(self, *a, _real=getattr(dist.BucketReducer, meth), _name="reducer." + meth):
            rec.add(_name, a)
            return _real(self, *a)
        mp.setattr(dist.BucketReducer, meth, traced)


def _names(rec, tr, batch):
    """Names that hold however the trainer files its activations: by layer and kind (aux / det_act / det_out per scale) or flat by
    name (act / det_out)."""
    for attr in ("P", "G", "Mo", "P16", "RS", "P_ema", "RS_ema", "z", "dz", "mean", "rstd", "ws", "wd_buf", "col", "zi", "xp", "dzp",
                 "loss_out", "grad_flat"):
        rec.walk(attr, getattr(tr, attr))
    acts = dict({"x0": tr.x0}, **{f"out{idx}": a for idx, a in tr.out.items()})
    if hasattr(tr, "aux"):
        for idx, a in tr.aux.items():
            acts.update({f"y{idx}": a["y"]}, **{f"t{idx}.{j}": t for j, t in enumerate(a.get("t", ()))})
            if "cat" in a:
                acts[f"cat{idx}"] = a["cat"]
        for s, d in enumerate(tr.det_act):
            acts.update({f"det{s}.{k}": a for k, a in d.items()})
        heads = {f"det{s}.{k}": t for s, d in enumerate(tr.det_out) for k, t in d.items()}
    else:
        acts.update(tr.act)
        heads = tr.det_out
    for name in sorted(acts):
        rec.walk(name, acts[name].buf)
    for name in sorted(heads):
        rec.walk(name, heads[name])
    rec.walk("", batch)


def record_case(case: str) -> dict:
    """{"allocs": {name: [shape, stride, dtype]}, "calls": [...]} of the case's steps."""
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    steps, kw = CASES[case]
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        for var in FLAGS:
            mp.delenv(var, raising=False)
        _patch(mp, rec)
        tr = YoloTrainer(init_yolo_train_state(SCALE, NC, seed=3), scale=SCALE, nc=NC, size=SIZE, batch=B, device="cpu", **kw)
        assert len(tr._phase_blocks) == (5 if kw.get("phase_dgrad") else 0)          # model.3, 5, 7, 16, 19: model.1 is too narrow
        g = torch.Generator().manual_seed(21)
        ctr, wh = torch.rand(B, GT, 2, generator=g) * (SIZE - 30) + 15, torch.rand(B, GT, 2, generator=g) * 20 + 8
        batch = dict(images=torch.randint(0, 256, (B, SIZE, SIZE, 3), generator=g, dtype=torch.uint8).as_subclass(_DeviceImages),
                     gt_boxes=torch.cat([ctr - wh / 2, ctr + wh / 2], -1),
                     gt_labels=torch.randint(0, NC, (B, GT), generator=g, dtype=torch.int32),
                     gt_counts=torch.full((B,), GT, dtype=torch.int32))
        _names(rec, tr, batch)
        rec.recording = True
        with tt._TorchOps(rec):
            for _ in range(steps):
                tr.step(batch["images"], batch["gt_boxes"], batch["gt_labels"], batch["gt_counts"])
        rec.recording = False
    return json.loads(json.dumps({"allocs": rec.alloc_table(), "calls": rec.trace}))


def fixture_path(case: str) -> str:
    return os.path.join(FIXTURE_DIR, case + ".json")


def load_fixture() -> dict:
    """{case: trace} of every file in the fixture directory."""
    out = {}
    for name in sorted(os.listdir(FIXTURE_DIR)):
        with open(os.path.join(FIXTURE_DIR, name), encoding="utf-8") as f:
            out.update(json.load(f))
    return out


if __name__ == "__main__":
    root = os.path.dirname(tt.HERE)
    sys.path[:0] = [root, os.path.join(root, "yolov8-vit_amd")]
    for case in CASES:
        text = tt.dumps({case: record_case(case)})
        if "--write" in sys.argv[1:]:
            os.makedirs(FIXTURE_DIR, exist_ok=True)
            with open(fixture_path(case), "w", encoding="utf-8") as f:
                f.write(text)
            print(f"wrote {fixture_path(case)}: {len(text)} bytes, {text.count(chr(10))} lines")
        else:
            sys.stdout.write(text)
