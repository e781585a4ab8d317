#!/usr/bin/env python3
"""Dev tool (GPU box): the YOLOv8m detector alone (YoloEngine("m", nc 80, 640 x 640), launch list + decode) at CDS_BATCH images
(default 64), unflagged and with dma32=True, alternating in one process: CDS_RUNS runs (default 3) of CDS_PASSES passes
(default 20) each, a run timed as one span between two stream events.  Prints ms per pass of every run.
YV_PKG names another checkout's package directory (the parent commit's, which has no dma32 flag: its unflagged runs only)."""
import inspect, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("YV_PKG", os.path.join(ROOT, "yolov8-vit_amd")))
import torch
from yvhip import engines

dev = "cuda:0"
B, RUNS, PASSES = (int(os.environ.get(k, d)) for k, d in (("CDS_BATCH", 64), ("CDS_RUNS", 3), ("CDS_PASSES", 20)))


def main():
    sd = engines.init_yolo_state("m", 80, 42, 4.0)
    plain = engines.YoloEngine(sd, "m", 80, 640, dev)
    states = {"unflagged": plain}
    if "dma32" in inspect.signature(engines.YoloEngine.__init__).parameters:
        flagged = plain.resized(640)
        flagged.dma32 = True
        states["dma32"] = flagged
    g = torch.Generator().manual_seed(1234)
    images = torch.randint(0, 256, (B, 640, 640, 3), generator=g, dtype=torch.uint8).to(dev)
    for eng in states.values():
        for _ in range(3):
            eng(images)
    torch.cuda.synchronize()
    ms = {k: [] for k in states}
    for _ in range(RUNS):
        for k, eng in states.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(PASSES):
                eng(images)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / PASSES)
    for k, v in ms.items():
        print(f"YOLOv8m detector, {B} images, {k:9s}: " + " / ".join(f"{x:.3f}" for x in v) + " ms per pass")


if __name__ == "__main__":
    main()
