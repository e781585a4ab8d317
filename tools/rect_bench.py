#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): what a rectangular network input buys the detect stage (YoloEngine +
efficient_nms) and the whole detect + classify pipeline.

  python3 tools/rect_bench.py                     every configuration below, one table
  python3 tools/rect_bench.py --trace n 384 640   20 detect-stage passes of YOLOv8n, 32 images, bf16 at 384 x 640 and nothing
                                                  else: the program to put behind `rocprofv3 --kernel-trace --stats --`
  python3 tools/rect_bench.py --layers A_kernel_trace.csv B_kernel_trace.csv
                                                  (no GPU) two such traces side by side, launch by launch: the passes are cut at
                                                  the stem kernel, the first one dropped, the rest averaged per position

Configurations: YOLOv8n at 32 images in bf16; YOLOv8m at 64 images in bf16 and mxfp8; extents 640 x 640, 480 x 640 and
384 x 640 (a 4:3 and a 16:9 photo letterboxed to the long side 640).  The engines of one configuration are siblings
(YoloEngine.resized: shared weights).  Every extent is warmed first; then the extents are timed ALTERNATELY inside one process,
RB_REPEATS (7) rounds of RB_CALLS (10) calls each between device events; a line gives the median round, the spread
(max - min) / median over the rounds and the ratio to the square's median, next to the ratio of the pixel counts.  The engine
is also timed without the NMS, whose time follows the candidates the random weights happen to give an extent, not its pixels.
End to end: DetectClassifyPipeline with ViT-B/16 at 4 crops per image on the YOLOv8n engines, the same way."""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolov8-vit_amd")):
    sys.path.insert(0, p)
import torch
import yvhip
from yvhip import engines
from yvhip.pipeline import DetectClassifyPipeline

DEV = "cuda:0"
REPEATS = int(os.environ.get("RB_REPEATS", 7))
CALLS = int(os.environ.get("RB_CALLS", 10))
EXTENTS = [(640, 640), (480, 640), (384, 640)]
CONFIGS = [("n", 32, "bf16"), ("m", 64, "bf16"), ("m", 64, "mxfp8")]


def round_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def alternate(fns):
    """fns {label: callable}: warm each, then REPEATS rounds, each round visiting every label once.  -> {label: [us per call]}"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            out[k].append(round_us(fn, CALLS))
    return out


def report(title, times):
    base = statistics.median(times[EXTENTS[0]])
    for hw in EXTENTS:
        t = times[hw]
        med = statistics.median(t)
        print(f"{title:34s} {hw[0]:3d} x {hw[1]:3d}  {med:9.1f} us  spread {100 * (max(t) - min(t)) / med:4.1f} %  "
              f"ratio {med / base:5.3f}  pixels {hw[0] * hw[1] / (EXTENTS[0][0] * EXTENTS[0][1]):5.3f}", flush=True)


def images(B, hw, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, *hw, 3), generator=g, dtype=torch.uint8).to(DEV)


def detect_pipes(scale, dtype, vits):
    sd = engines.init_yolo_state(scale, 5, 42, 4.0)
    base = engines.YoloEngine(sd, scale, 5, 640, DEV, dtype=dtype)
    return {hw: DetectClassifyPipeline(base if hw == (640, 640) else base.resized(hw), vits, max_crops_per_image=4)
            for hw in EXTENTS}


def passes(path):
    """Kernel trace CSV -> [[(kernel, workgroups, us)] per detect-stage pass], cut at the stem kernel, last dispatch = the crop
    compaction; the first pass (warm-up) dropped."""
    rows = sorted(csv.DictReader(open(path, newline="")), key=lambda r: int(r["Start_Timestamp"]))
    out, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "stem_mfma_kernel" in name:
            cur = []
            out.append(cur)
        if cur is None:
            continue
        short = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
        wgs = 1
        for ax in "XYZ":
            wgs *= max(int(r[f"Grid_Size_{ax}"]) // max(int(r[f"Workgroup_Size_{ax}"]), 1), 1)
        cur.append((short[:44], wgs, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        if "compact_crops_kernel" in name:
            cur = None
    return out[1:]


def layers(path_a, path_b):
    pa, pb = passes(path_a), passes(path_b)
    n = len(pa[0])
    assert all(len(p) == n for p in pa + pb), "the two traces hold different launch lists"
    print(f"# {len(pa)} / {len(pb)} passes averaged; us per launch, workgroups per launch")
    print(f"{'#':>3s} {'kernel':44s} {'wgs A':>7s} {'us A':>8s} {'wgs B':>7s} {'us B':>8s} {'B / A':>6s}")
    ta = tb = 0.0
    for i in range(n):
        a = statistics.mean(p[i][2] for p in pa)
        b = statistics.mean(p[i][2] for p in pb)
        ta, tb = ta + a, tb + b
        print(f"{i:3d} {pa[0][i][0]:44s} {pa[0][i][1]:7d} {a:8.1f} {pb[0][i][1]:7d} {b:8.1f} {b / a:6.2f}")
    print(f"{'':3s} {'sum of kernel times':44s} {'':7s} {ta:8.1f} {'':7s} {tb:8.1f} {tb / ta:6.2f}")


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--layers":
        return layers(sys.argv[2], sys.argv[3])
    yvhip.require_gpu()
    name = "vit_base_patch16_224"
    vits = [engines.VitEngine(engines.init_vit_wrapper_state(name, 5, 42), name, 5, device=DEV)]
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        scale = sys.argv[2]
        B = dict((s, b) for s, b, _ in CONFIGS)[scale]
        hw = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (384, 640)
        pipe, img = detect_pipes(scale, "bf16", vits)[hw], images(B, hw)
        for _ in range(int(os.environ.get("PASSES", 20))):
            det = pipe.detect_stage(img)
        torch.cuda.synchronize()
        print("crops:", int(det["crop_total"]))
        return
    print(f"# {REPEATS} rounds of {CALLS} calls per extent, extents alternated; us per call = median round", flush=True)
    for scale, B, dtype in CONFIGS:
        pipes = detect_pipes(scale, dtype, vits)
        imgs = {hw: images(B, hw) for hw in EXTENTS}
        times = alternate({hw: (lambda hw=hw: pipes[hw].detect_stage(imgs[hw])) for hw in EXTENTS})
        report(f"detect stage YOLOv8{scale} B={B} {dtype}", times)
        times = alternate({hw: (lambda hw=hw: pipes[hw].yolo(imgs[hw])) for hw in EXTENTS})
        report(f"engine alone YOLOv8{scale} B={B} {dtype}", times)
        if (scale, dtype) == ("n", "bf16"):
            times = alternate({hw: (lambda hw=hw: pipes[hw](imgs[hw])) for hw in EXTENTS})
            report(f"end to end YOLOv8n + ViT-B/16 B={B}", times)
            crops = {hw: int(pipes[hw](imgs[hw])["crop_total"][0]) for hw in EXTENTS}
            print(f"# crops classified per batch: {crops}", flush=True)


if __name__ == "__main__":
    main()
