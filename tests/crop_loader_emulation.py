"""TEST INFRASTRUCTURE ONLY: numpy statement of `yv_train_crops` (csrc/train_crops.hip) and a seeded dataset writer for the
device crop loader tests.

`virtual_crop` states, with the clamps include/yv_hip.h documents, which pool byte a tap of the S x S crop reads; for a plan
row whose rectangle lies inside its image it equals oracle.boxes.crop_resize_normalize.  `train_crops_reference` is that
followed by oracle.augment.apply_record, i.e. the composition the kernel must match bit for bit."""
import math
import os

import numpy as np

from oracle import augment as oa
from oracle import boxes as ob

MAX_DIM = 1 << 24


def _nearest(m, dst, src):
    """oracle.boxes.nearest_index_table(dst, src)[m] for int arrays m, any src >= 1 (f64, one rounding per operation)."""
    ifx = 1.0 / (float(dst) / float(src))
    return np.array([min(int(math.floor(int(d) * ifx)), src - 1) for d in m], dtype=np.int64)


def folded_tables(table, plan_row, idx_row, S):
    """Source column / row of every entry of the record's integer tables (the kernel builds these in LDS)."""
    n = table.shape[0]
    img = int(np.clip(plan_row[0], 0, n - 1))
    off = int(table[img, 0])
    W, H = int(np.clip(table[img, 1], 1, MAX_DIM)), int(np.clip(table[img, 2], 1, MAX_DIM))
    x0, y0, x1, y1 = (int(v) for v in plan_row[1:5])
    cw, ch = max(x1 - x0, 1), max(y1 - y0, 1)
    mapx = np.clip(np.asarray(idx_row[36:36 + S], dtype=np.int64), 0, S - 1)
    mapy = np.clip(np.asarray(idx_row[36 + S:36 + 2 * S], dtype=np.int64), 0, S - 1)
    col = np.clip(x0 + _nearest(mapx, S, cw), 0, W - 1)
    row = np.clip(y0 + _nearest(mapy, S, ch), 0, H - 1)
    return off, W, col, row


def virtual_crop(pool, table, plan_row, S):
    """(3,S,S) f32: the normalised crop whose taps the kernel reads (identity tables), clamps included."""
    ident = np.zeros(36 + 2 * S, dtype=np.int64)
    ident[36:36 + S] = ident[36 + S:] = np.arange(S)
    off, W, col, row = folded_tables(table, plan_row, ident, S)
    off = int(np.clip(off, 0, pool.size))
    addr = np.clip(off + 3 * (row[:, None] * W + col[None, :]), 0, pool.size - 3)
    px = np.stack([pool[addr + c] for c in range(3)])
    return ob.normalize_u8(px)


def train_crops_reference(pool, table, plan, geo, idx, S, P, layout):
    """layout 2: (B*(S/P)^2, 3*P*P) f32 holding bf16-rounded values; layout 0: (B,3,S,S) f32 (records must be identity)."""
    outs = []
    for b in range(plan.shape[0]):
        x = virtual_crop(pool, table, plan[b], S)
        outs.append(oa.apply_record(x, geo[b], idx[b], P) if layout == 2 else x[None])
    return np.concatenate(outs)


# ------------------------------------------------------------------------------------------------ dataset on disk
CLASSES = ["good", "broke", "lose", "uncovered", "circle"]


def _xml(fname, objs):
    body = "".join(f"<object><name>{n}</name><bndbox><xmin>{a}</xmin><ymin>{b}</ymin><xmax>{c}</xmax><ymax>{d}</ymax></bndbox></object>"
                   for n, (a, b, c, d) in objs)
    return f"<annotation><filename>{fname}</filename><path>{fname}</path>{body}</annotation>"


def write_dataset(root, seed=0, n_images=7, sizes=None, many=9):
    """VOC xml + image pairs directly inside `root`: mixed sizes, PNG and JPEG, image 0 with `many` objects, boxes that touch
    every border, a 1-pixel-wide and a 1-pixel-high box, several circles.  Returns the directory as str."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    sizes = sizes or [(97, 61), (320, 200), (64, 128), (500, 375), (33, 47), (256, 256), (131, 77), (640, 360)]
    for i in range(n_images):
        w, h = sizes[i % len(sizes)]
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        fname = f"s{seed}_{i}." + ("jpg" if i % 2 else "png")
        Image.fromarray(img).save(os.path.join(root, fname), **({"quality": 90} if i % 2 else {}))
        objs = []
        for k in range(many if i == 0 else 1 + i % 3):
            bw, bh = int(rng.integers(4, max(w // 2, 6))), int(rng.integers(4, max(h // 2, 6)))
            x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
            objs.append((CLASSES[(i + k) % 5], (x0, y0, x0 + bw, y0 + bh)))
        if i == 1:
            objs += [("good", (0, 0, w, h)), ("broke", (0, 5, 30, h)), ("lose", (w - 25, 0, w, 20)), ("circle", (0, h - 12, w, h))]
        if i == 2:
            objs += [("uncovered", (10, 3, 11, 90)), ("circle", (2, 40, 60, 41)), ("good", (w - 1, 0, w, h))]
        with open(os.path.join(root, os.path.splitext(fname)[0] + ".xml"), "w") as f:
            f.write(_xml(fname, objs))
    return str(root)
