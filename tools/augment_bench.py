"""Times the augmentation gather kernels against their HBM roofline (algorithmic bytes / time): the classifier's
`augment_patchify`, the detector's `mosaic_augment` and, alternating with it in the same process, `mosaic_augment_ex` on
the same affine records, with every geometric knob on, and with two layers (mixup).
    python tools/augment_bench.py            (on the GPU box)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import yvhip                                                   # noqa: E402
from yvhip.augment import TrainAugment                         # noqa: E402
from yvhip.yolo_augment import DetAugment, batch_records_ex, build_record, tile_geometry   # noqa: E402

DEV = "cuda:0"


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3                         # us


def ex_records(plans, sizes, S):
    """Device tensors of one `mosaic_augment_ex` call for `plans` (tile k holds source k); mix is None with one layer."""
    rec_h, rec_i, mix, lut = batch_records_ex(plans, dict(enumerate(sizes)), {k: k for k in range(len(sizes))}, S)
    t = [torch.from_numpy(a).to(DEV) for a in (rec_h, rec_i, mix, lut)]
    return t[0], t[1], (t[2] if rec_h.shape[1] == 2 else None), t[3]


def main():
    yvhip.require_gpu()
    S, P, B = 224, 16, 256                                     # classifier crops: (B,3,S,S) f32 in, bf16 patch rows out
    x = torch.randn(B, 3, S, S, device=DEV)
    geo, idx = TrainAugment(S, seed=1).sample(B)
    geo, idx = torch.from_numpy(geo).to(DEV), torch.from_numpy(idx).to(DEV)
    out = torch.empty((B * (S // P) ** 2, 3 * P * P), dtype=torch.bfloat16, device=DEV)
    us = timeit(lambda: yvhip.augment_patchify(x, geo, idx, P, out))
    alg = B * 3 * S * S * (4 + 2)
    print(f"augment_patchify  B={B} S={S}: {us:8.1f} us  {alg / us / 1e3:7.1f} GB/s algorithmic ({alg / 1e6:.1f} MB)")
    from yvhip.modules import patchify_bf16
    us0 = timeit(lambda: patchify_bf16(x, P))
    print(f"  torch patchify_bf16 (no augmentation) for scale: {us0:8.1f} us")

    S, B, n_tiles = 640, 16, 40                                # detector inputs: 4 tiles per output image
    rng = np.random.default_rng(0)
    sizes = [tile_geometry(int(rng.integers(300, 1400)), int(rng.integers(300, 1400)), S) for _ in range(n_tiles)]
    tiles = torch.randint(0, 256, (n_tiles, S, S, 3), dtype=torch.uint8, device=DEV)
    aug = DetAugment(S, seed=2)
    plans = [aug.plan(b, n_tiles) for b in range(B)]
    rf, ri, lut = [], [], []
    for p in plans:
        f, i, l, _, _, _ = build_record(p, [sizes[s] for s in p["sources"]], p["sources"], S)
        rf.append(f); ri.append(i); lut.append(l)
    rf, ri, lut = (torch.from_numpy(np.stack(a)).to(DEV) for a in (rf, ri, lut))
    us = timeit(lambda: yvhip.mosaic_augment(tiles, rf, ri, lut))
    alg = B * S * S * 3 * 2                                    # one source byte (at scale 1) + one output byte per value
    print(f"mosaic_augment    B={B} S={S}: {us:8.1f} us  {alg / us / 1e3:7.1f} GB/s algorithmic ({alg / 1e6:.1f} MB)")

    # the non-default knobs: four variants alternating in this process, median of the rounds against mosaic_augment's
    affine = ex_records(plans, sizes, S)                       # the same plans: last row (0, 0, 1), one layer
    assert torch.equal(yvhip.mosaic_augment_ex(tiles, *affine), yvhip.mosaic_augment(tiles, rf, ri, lut))
    geo = DetAugment(S, seed=2, degrees=45.0, shear=10.0, perspective=0.001, flipud=0.5)
    knobs = ex_records([geo.plan(b, n_tiles) for b in range(B)], sizes, S)
    mixed = DetAugment(S, seed=2, degrees=45.0, shear=10.0, perspective=0.001, flipud=0.5, mixup=1.0)
    two = ex_records([mixed.plan(b, n_tiles) for b in range(B)], sizes, S)
    variants = [
        ("mosaic_augment", lambda: yvhip.mosaic_augment(tiles, rf, ri, lut)),
        ("mosaic_augment_ex affine, 1 layer", lambda: yvhip.mosaic_augment_ex(tiles, *affine)),
        ("mosaic_augment_ex all knobs, 1 layer", lambda: yvhip.mosaic_augment_ex(tiles, *knobs)),
        ("mosaic_augment_ex all knobs, 2 layers", lambda: yvhip.mosaic_augment_ex(tiles, *two)),
    ]
    rounds = [[timeit(fn, n=200) for _, fn in variants] for _ in range(9)]
    med = np.median(np.asarray(rounds), axis=0)
    print(f"detector augmentation, B={B} S={S}, 9 alternating rounds of 200 calls (us per call: median [min, max], x mosaic_augment):")
    for k, (name, _) in enumerate(variants):
        col = [r[k] for r in rounds]
        print(f"  {name:40s} {med[k]:8.1f} [{min(col):7.1f}, {max(col):7.1f}]  x{med[k] / med[0]:.2f}")


if __name__ == "__main__":
    main()
