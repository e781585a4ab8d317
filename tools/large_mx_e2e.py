#!/usr/bin/env python3
"""A/B of the MXFP8 detector (YoloEngine(dtype="mxfp8")) against the bf16 detector on the BASELINE.json configs[4] set-up of
`bench.py --models large --batch 64 --dtype mxfp8`: YOLOv8m + ViT-L/16 (MXFP8 block linears), 640 x 640, 4 crops per image,
PipelinedRunner with the split classifier, seeded random weights and images as bench.py builds them.  Both pipelines are
built once in one process and timed alternately (ROUNDS rounds of STEPS steps each after WARMUP steps), then the detect
stage alone (pipe.detect_stage) the same way.  Prints one JSON line per measurement."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch

from yvhip import engines
from yvhip.pipeline import DetectClassifyPipeline, PipelinedRunner

STEPS, WARMUP, ROUNDS = int(os.environ.get("STEPS", 10)), int(os.environ.get("WARMUP", 3)), int(os.environ.get("ROUNDS", 3))
B, R, dev = int(os.environ.get("BATCH", 64)), 4, "cuda:0"
vit_name = "vit_large_patch16_224"
yolo_sd = engines.init_yolo_state("m", 5, seed=42, head_gain=4.0)
vit = engines.VitEngine(engines.init_vit_wrapper_state(vit_name, 5, seed=42), vit_name, 5, device=dev, dtype="mxfp8")
pipes = {}
for dt in ("bf16", "mxfp8"):
    pipe = DetectClassifyPipeline(engines.YoloEngine(yolo_sd, "m", 5, 640, device=dev, dtype=dt), [vit], max_crops_per_image=R)
    pipes[dt] = (pipe, PipelinedRunner(pipe, split_classifier=True))
g = torch.Generator().manual_seed(1234)
images = torch.randint(0, 256, (B, 640, 640, 3), generator=g, dtype=torch.uint8).to(dev)


def timed(fn, n):
    for _ in range(WARMUP):
        out = fn(images)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn(images)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


for what in ("e2e", "detect"):
    for r in range(ROUNDS):
        for dt in ("bf16", "mxfp8"):
            pipe, runner = pipes[dt]
            fn = runner.submit if what == "e2e" else pipe.detect_stage
            sec, out = timed(fn, STEPS)
            rec = {"what": what, "detector": dt, "round": r, "batch": B, "ms_per_step": round(sec * 1e3, 3),
                   "images_per_s": round(B / sec, 1), "crops_per_step": int(out["crop_total"][0])}
            if what == "e2e":
                rec["mx_layers"] = len(pipe.yolo.mx_layers)
            print(json.dumps(rec), flush=True)
