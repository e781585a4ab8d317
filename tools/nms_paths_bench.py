#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): time yvhip.efficient_nms on inputs that leave the head of the multi-workgroup
form for the general path (exact top-k select, heavy classes, in-place compaction) - bench.py --mode postproc times only images
the head finishes.

  python3 tools/nms_paths_bench.py [case ...]     default: one_class_select atomic_list_head44 atomic_list_no_head multichunk_compaction

The cases are those of tests/nms_cases.py, their images repeated to a batch of 32.  Each case is checked against itself first
(both device forms give the same four outputs), warmed, then timed with device events in batches of calls until it has at
least NPB_SECONDS (0.3) of calls; the figure is the median batch.  One line per case: us per call of the multi-workgroup form
and of the single-workgroup form."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolov8-vit_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import yvhip
import nms_cases

yvhip.require_gpu()
dev = "cuda:0"
SECONDS = float(os.environ.get("NPB_SECONDS", 0.3))
IMAGES = 32
DEFAULT = ["one_class_select", "atomic_list_head44", "atomic_list_no_head", "multichunk_compaction"]


def batch_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def median_us(fn):
    for _ in range(5):
        fn()
    n = max(4, int(0.02e6 / max(batch_us(fn, 4), 1.0)))          # ~20 ms of calls per batch
    batches, spent = [], 0.0
    while spent < SECONDS * 1e6 or len(batches) < 5:
        batches.append(batch_us(fn, n))
        spent += batches[-1] * n
    return statistics.median(batches), len(batches) * n


def main(names):
    for name in names:
        boxes, scores = nms_cases.case_inputs(name)
        kw = nms_cases.CASES[name][1]
        rep = (IMAGES + boxes.shape[0] - 1) // boxes.shape[0]
        b = boxes.repeat(rep, 1, 1)[:IMAGES].contiguous().to(dev)
        s = scores.repeat(rep, 1, 1)[:IMAGES].contiguous().to(dev)
        args = (kw.get("thr", 0.25), kw.get("iou", 0.65), kw.get("max_out", 100), kw.get("topk", 4096))
        multi = lambda: yvhip.efficient_nms(b, s, *args)
        single = lambda: yvhip.efficient_nms(b, s, *args, single_kernel=True)
        for x, y in zip(multi(), single()):
            assert torch.equal(x, y), name
        (tm, nm), (ts, ns) = median_us(multi), median_us(single)
        print(f"{name:24s} {IMAGES} x {boxes.shape[1]} x {scores.shape[2]}  multi-workgroup {tm:8.1f} us ({nm} calls)  "
              f"single-workgroup {ts:8.1f} us ({ns} calls)  kept {int(multi()[0].sum())}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or DEFAULT)
