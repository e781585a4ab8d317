#!/usr/bin/env python3
"""Accuracy of YoloEngine(dtype="mxfp8") against the bf16 engine for candidate layer plans (the measurement behind
engines.MX_MIN_WIDTH): per scale, seeded random weights (head_gain 4) and two 640 x 640 images as
tests/test_gpu_conv_mx.py::test_yolo_engine_mxfp8_tracks_bf16 uses; for each minimum layer width (and with / without the head's
3 x 3 layers) the plan size, the logits' rel-L2 (max over the six per-scale tensors) and the smallest per-anchor cosine."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import torch.nn.functional as F

from yvhip import engines

dev = "cuda:0"
plan0 = engines.mx_conv_plan
for scale in "nsm":
    sd = engines.init_yolo_state(scale, 5, seed=7, head_gain=4.0)
    e16 = engines.YoloEngine(sd, scale, 5, 640, dev)
    g = torch.Generator().manual_seed(8)
    img = torch.randint(0, 256, (2, 640, 640, 3), generator=g, dtype=torch.uint8).to(dev)
    b16, c16 = e16.forward_raw(img)
    for mw in (0, 64, 96, 128):
        for head in (True, False):
            keys = [k for k in plan0(scale, 5, min_width=mw) if head or not (k.startswith("det") or k.startswith("model.22."))]
            engines.mx_conv_plan = lambda s, nc, *a, _k=keys, **kw: list(_k)
            e8 = engines.YoloEngine(sd, scale, 5, 640, dev, dtype="mxfp8")
            engines.mx_conv_plan = plan0
            b8, c8 = e8.forward_raw(img)
            rel, cos = 0.0, []
            for p16, p8 in ((b16, b8), (c16, c8)):
                for a, b in zip(p16, p8):
                    a, b = a.double().flatten(0, 2), b.double().flatten(0, 2)
                    rel = max(rel, float((b - a).norm() / a.norm()))
                    cos.append(F.cosine_similarity(a, b, dim=1))
            cos = torch.cat(cos)
            print(f"YOLOv8{scale} min_width {mw:3d} head {'mx  ' if head else 'bf16'} MX layers {len(keys):3d}: rel-L2 {rel:.4f}, "
                  f"per-anchor cosine min {float(cos.min()):.5f}, 1 % quantile {float(torch.quantile(cos.float().cpu(), 0.01)):.5f}",
                  flush=True)
            del e8
