"""Epoch throughput of utils.trainClass.train_one_epoch with the host loader against the device-resident crop loader
(build_dataloader(device_pool=True), yvhip/crop_loader.py, csrc/train_crops.hip), DESIGN.md section 12.

A seeded synthetic dataset is written to a temporary directory (JPEG and PNG files of mixed sizes up to 1920 x 1080, VOC xml
with several objects per image).  Whole epochs are timed ALTERNATELY, host loader then device loader, --reps times, after one
untimed epoch of each; every run ends in a device synchronise.  One JSON line per run (crops/s), then a summary line with the
pool build time and bytes (paid once per training run, reported separately), the bare step rate (VitTrainer.step on a resident
batch: the ceiling) and a per-batch split of the device loader's host work.

    python tools/train_loader_bench.py
    rocprofv3 --kernel-trace --stats -d prof -o tl -- python tools/train_loader_bench.py --kernels      (kernel times only)
"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolov8-vit_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [(1920, 1080), (1280, 720), (1600, 1200), (800, 600), (1024, 768), (640, 480), (1920, 1080), (1366, 768)]
CLASSES = ["good", "broke", "lose", "uncovered", "circle"]


def write_dataset(root, n_images, n_objects, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for i in range(n_images):
        w, h = SIZES[i % len(SIZES)]
        coarse = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)          # blocky, so the files compress
        img = np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1)[:h, :w]
        fname = f"img{i}." + ("png" if i % 4 == 3 else "jpg")
        Image.fromarray(img).save(os.path.join(root, fname))
        objs = ""
        for k in range(n_objects):
            bw, bh = int(rng.integers(60, w // 3)), int(rng.integers(60, h // 3))
            x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            objs += (f"<object><name>{CLASSES[(i + k) % 5]}</name><bndbox><xmin>{x0}</xmin><ymin>{y0}</ymin><xmax>{x0 + bw}</xmax>"
                     f"<ymax>{y0 + bh}</ymax></bndbox></object>")
        with open(os.path.join(root, f"img{i}.xml"), "w") as f:
            f.write(f"<annotation><filename>{fname}</filename><path>{fname}</path>{objs}</annotation>")


def timed_us(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def kernel_pair(pool, B=256, S=224, P=16):
    """yv_train_crops against yv_augment_patchify for the same B crops and records (event-timed; a profiler sees both)."""
    import yvhip
    from yvhip.augment import TrainAugment
    from yvhip.crop_loader import CropBatch
    rng = np.random.default_rng(3)
    plan = []
    for _ in range(B):
        i = int(rng.integers(0, len(pool)))
        w, h = pool.sizes[i]
        bw, bh = int(rng.integers(60, w // 3)), int(rng.integers(60, h // 3))
        x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
        plan.append((i, x0, y0, x0 + bw, y0 + bh))
    plan = torch.tensor(plan, dtype=torch.int32, device=pool.device)
    geo, idx = TrainAugment(S, seed=1).sample(B)
    x = CropBatch(pool, plan.cpu().numpy(), S).images()                          # the f32 batch the old kernel starts from
    geo, idx = torch.from_numpy(geo).to(pool.device), torch.from_numpy(idx).to(pool.device)
    out = torch.empty((B * (S // P) ** 2, 3 * P * P), dtype=torch.bfloat16, device=pool.device)
    new = timed_us(lambda: yvhip.train_crops(pool.pool, pool.table, plan, geo, idx, S, P, 2, out))
    old = timed_us(lambda: yvhip.augment_patchify(x, geo, idx, P, out))
    assert torch.equal(yvhip.train_crops(pool.pool, pool.table, plan, geo, idx, S, P), yvhip.augment_patchify(x, geo, idx, P))
    return {"kernel_pair": {"crops": B, "S": S, "P": P, "train_crops_us": round(new, 1), "augment_patchify_us": round(old, 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", default="vit_base_patch16_224")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--kernels", action="store_true", help="only the kernel pair (profiler runs)")
    a = ap.parse_args()
    import utils.trainClass as tc
    import yvhip
    from yvhip.crop_loader import DevicePool
    from yvhip.modules import Network_Wrapper, create_model
    yvhip.require_gpu()
    tc.CFG.train_bs, tc.CFG.valid_bs = a.batch, a.batch
    dev = tc.CFG.device
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, a.images, a.objects, a.seed)
        random.seed(a.seed)
        objs, circ = tc.xml2pd([root])
        n = len(objs) + len(circ)
        t0 = time.perf_counter()
        pool = DevicePool([o["path"] for o in objs + circ], device=dev)
        torch.cuda.synchronize()
        pool_s = time.perf_counter() - t0
        if a.kernels:
            print(json.dumps(kernel_pair(pool)), flush=True)
            return
        net = Network_Wrapper(create_model(a.model, pretrained=False, num_classes=1000), tc.CFG.num_classes).to(dev)

        def epoch(device_loader, rep):
            tc.set_seed(a.seed + rep)
            tf = tc.build_transforms(tc.CFG)
            loader, _ = tc.build_dataloader(objs, circ, [], [], tf, **({"device_pool": pool} if device_loader else {}))
            torch.cuda.synchronize()
            t = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                tc.train_one_epoch(net, None, loader, tc.build_loss, None, [1e-4], a.batch, 0, 2, True, dev)
            torch.cuda.synchronize()
            return time.perf_counter() - t

        steps = n // a.batch
        for dl in (False, True):                                   # untimed: trainer construction, first-use allocations
            epoch(dl, -1)
        rates = {False: [], True: []}
        for rep in range(a.reps):
            for dl in (False, True):
                s = epoch(dl, rep)
                rates[dl].append(steps * a.batch / s)
                print(json.dumps({"loader": "device" if dl else "host", "rep": rep, "epoch_s": round(s, 4), "steps": steps,
                                  "crops_per_s": round(rates[dl][-1], 1)}), flush=True)
        # ceiling: the native step on a resident batch
        tr = net._yv_trainer
        P = tr.P_
        pm = torch.zeros((a.batch * (224 // P) ** 2, 3 * P * P), dtype=torch.bfloat16, device=dev)
        labels = torch.zeros((a.batch,), dtype=torch.int32, device=dev)
        step_us = timed_us(lambda: tr.step(pm, labels, 1e-4), n=10)
        # where a device-loader batch spends its host time
        tc.set_seed(a.seed)
        tf = tc.build_transforms(tc.CFG)
        loader, _ = tc.build_dataloader(objs, circ, [], [], tf, device_pool=pool)
        t = time.perf_counter()
        batches = [b for b in loader if b[0].shape[0] == a.batch]
        plan_ms = (time.perf_counter() - t) / max(len(batches), 1) * 1e3
        t = time.perf_counter()
        recs = [tf["train"].device_augment.sample(a.batch) for _ in batches]
        rec_ms = (time.perf_counter() - t) / max(len(batches), 1) * 1e3
        torch.cuda.synchronize()
        t = time.perf_counter()
        for (b, _, _), (geo, idx) in zip(batches, recs):
            b.patch_operand(geo, idx, P)
        torch.cuda.synchronize()
        op_ms = (time.perf_counter() - t) / max(len(batches), 1) * 1e3
        t = time.perf_counter()
        net.load_state_dict(tr.state_dict())
        torch.cuda.synchronize()
        sync_ms = (time.perf_counter() - t) * 1e3
        med = {k: statistics.median(v) for k, v in rates.items()}
        out = {"model": a.model, "batch": a.batch, "images": a.images, "crops_per_epoch": n, "steps_per_epoch": steps,
               "host_crops_per_s": round(med[False], 1), "host_crops_per_s_all": [round(v, 1) for v in rates[False]],
               "device_crops_per_s": round(med[True], 1), "device_crops_per_s_all": [round(v, 1) for v in rates[True]],
               "speedup": round(med[True] / med[False], 2), "pool_build_s": round(pool_s, 3), "pool_bytes": pool.nbytes,
               "bare_step_ms": round(step_us / 1e3, 3), "bare_step_crops_per_s": round(a.batch / (step_us * 1e-6), 1),
               "device_share_of_bare_step": round(med[True] / (a.batch / (step_us * 1e-6)), 3),
               "per_batch_ms": {"plan_from_loader": round(plan_ms, 3), "draw_records": round(rec_ms, 3),
                                "h2d_plus_train_crops": round(op_ms, 3)},
               "per_epoch_ms": {"load_state_dict": round(sync_ms, 3)}}
        out.update(kernel_pair(pool))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
