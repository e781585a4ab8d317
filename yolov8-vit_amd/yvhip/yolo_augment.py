"""Host side of the detector's training augmentation: what `model.train(...)` of
utils/trainYolo.py:28 applies - Mosaic(p 1.0, four images around a random centre of a 2S canvas) ->
RandomPerspective(degrees, translate 0.1, scale 0.5, shear, perspective) -> MixUp -> RandomHSV(0.015, 0.7, 0.4) ->
RandomFlip(ud, lr 0.5); without mosaic (`close_mosaic` epochs): LetterBox -> the same transform on the S canvas, no MixUp.
degrees, shear, perspective, flipud and mixup are 0 in the published defaults; copy-paste is not built (no instance masks).

The host draws the random numbers, decodes the files and transforms the LABELS (a few boxes per image); every pixel
is produced on the device: sources are resized by `yv_letterbox` into S x S tiles and one gather pass per output image
reads them through the inverse map (the 2S x 2S canvas is never materialised): `yv_mosaic_augment` (inverse affine) while
every plan of the batch is free of the non-default features, `yv_mosaic_augment_ex` (inverse homography, two flip bits, an
optional second layer blended in) otherwise.  Parity unpinned: the pipeline lives in `ultralytics` / OpenCV (absent);
8-bit HSV, the bilinear rounding, the `w <= 0` fill rule and the 8-bit layers of the blend are this build's own statements
(oracle/yolo_augment.py), which can differ from OpenCV's fixed-point paths by one grey level.
"""
from __future__ import annotations

import math
import os
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import YvError

FILL = 114


def tile_geometry(w0: int, h0: int, S: int) -> Tuple[int, int]:
    """Size of a source after the loader's resize: long side -> S, ceil, capped at S."""
    r = S / max(h0, w0)
    if r == 1:
        return w0, h0
    return min(math.ceil(w0 * r), S), min(math.ceil(h0 * r), S)


def mosaic_placement(i: int, xc: int, yc: int, w: int, h: int, S: int):
    """Canvas rectangle (x1a,y1a,x2a,y2a) of quadrant i (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right) around
    the centre (xc,yc) of the 2S canvas and the tile pixel (x1b,y1b) shown at its top-left corner."""
    s2 = 2 * S
    if i == 0:
        x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
        x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
    elif i == 1:
        x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s2), yc
        x1b, y1b = 0, h - (y2a - y1a)
    elif i == 2:
        x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s2, yc + h)
        x1b, y1b = w - (x2a - x1a), 0
    else:
        x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s2), min(s2, yc + h)
        x1b, y1b = 0, 0
    return (x1a, y1a, x2a, y2a), (x1b, y1b)


def affine_matrix(canvas: int, S: int, scale: float, tx: float, ty: float) -> np.ndarray:
    """Forward 3x3 matrix T @ R @ C of RandomPerspective with degrees = shear = perspective = 0: centre the canvas,
    scale, translate by (tx, ty) * S."""
    C = np.array([[1, 0, -canvas / 2], [0, 1, -canvas / 2], [0, 0, 1]], dtype=np.float64)
    R = np.diag([scale, scale, 1.0])
    T = np.array([[1, 0, tx * S], [0, 1, ty * S], [0, 0, 1]], dtype=np.float64)
    return T @ R @ C


def forward_matrix(canvas: int, S: int, scale: float, tx: float, ty: float, angle: float = 0.0,
                   shear: Tuple[float, float] = (0.0, 0.0), perspective: Tuple[float, float] = (0.0, 0.0)) -> np.ndarray:
    """Forward 3x3 matrix T @ Sh @ R @ P @ C of RandomPerspective.affine_transform: C and T as in `affine_matrix`, P the
    identity with P[2,0], P[2,1] = perspective, R = getRotationMatrix2D(angle in degrees, about the origin, scale) (a
    positive angle turns the displayed image counter-clockwise), Sh the identity with Sh[0,1] = tan(shear x),
    Sh[1,0] = tan(shear y) (degrees).  With angle, shear and perspective 0 it is `affine_matrix`, bit for bit."""
    if angle == 0 and tuple(shear) == (0, 0) and tuple(perspective) == (0, 0):
        return affine_matrix(canvas, S, scale, tx, ty)
    C = np.array([[1, 0, -canvas / 2], [0, 1, -canvas / 2], [0, 0, 1]], dtype=np.float64)
    P = np.eye(3)
    P[2, 0], P[2, 1] = perspective
    a = math.radians(angle)
    R = np.array([[scale * math.cos(a), scale * math.sin(a), 0], [-scale * math.sin(a), scale * math.cos(a), 0], [0, 0, 1]],
                 dtype=np.float64)
    Sh = np.eye(3)
    Sh[0, 1], Sh[1, 0] = math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1]))
    T = np.array([[1, 0, tx * S], [0, 1, ty * S], [0, 0, 1]], dtype=np.float64)
    return T @ Sh @ R @ P @ C


def layer_matrix(layer: dict, canvas: int, S: int) -> np.ndarray:
    """`forward_matrix` of one geometric plan (a plan, or its `mix` entry); absent keys are 0."""
    return forward_matrix(canvas, S, layer["scale"], *layer["translate"], angle=layer.get("angle", 0.0),
                          shear=layer.get("shear", (0.0, 0.0)), perspective=layer.get("perspective", (0.0, 0.0)))


def homography_record(M: np.ndarray) -> np.ndarray:
    """Forward matrix -> the nine f32 of `yv_mosaic_augment_ex`: inv(M) normalised to [2,2] = 1.  An affine M (last row
    exactly (0, 0, 1)) keeps its inverse as computed - whose [2,2] is 1 - and gets the last row (0, 0, 1) exactly, so
    the first six floats are `build_record`'s rec_f."""
    H = np.linalg.inv(M)
    if M[2, 0] == 0 and M[2, 1] == 0 and M[2, 2] == 1:
        H[2] = (0.0, 0.0, 1.0)
    else:
        H = H / H[2, 2]
    return H.reshape(-1).astype(np.float32)


def hsv_tables(gains: Sequence[float]) -> np.ndarray:
    """(3,256) u8 tables of RandomHSV: hue (x * r0) % 180, saturation / value clip(x * r, 0, 255)."""
    x = np.arange(256, dtype=np.float64)
    return np.stack([(x * gains[0]) % 180, np.clip(x * gains[1], 0, 255), np.clip(x * gains[2], 0, 255)]).astype(np.uint8)


def transform_boxes(boxes: np.ndarray, labels: np.ndarray, M: np.ndarray, scale: float, S: int, flip: bool, flipud: bool = False):
    """xyxy boxes on the canvas -> boxes on the output: the four corners through M (with the homogeneous divide when M's
    last row is not (0, 0, 1); a box with a corner at w <= 0 is dropped), clip to [0,S], the candidate filter (both
    sides > 2 px, area kept > 10 %, aspect ratio < 100 - against the pre-transform box times `scale`), flips."""
    if len(boxes) == 0:
        return np.zeros((0, 4), np.float32), np.zeros((0,), np.int32)
    b = boxes.astype(np.float64)
    corners = np.stack([b[:, [0, 1]], b[:, [2, 3]], b[:, [0, 3]], b[:, [2, 1]]], axis=1)           # (n,4,2)
    if M[2, 0] == 0 and M[2, 1] == 0 and M[2, 2] == 1:
        pts = corners @ M[:2, :2].T + M[:2, 2]
    else:
        w = corners @ M[2, :2] + M[2, 2]                                                             # (n,4)
        front = (w > 0).all(axis=1)
        b, corners, w, labels = b[front], corners[front], w[front], labels[front]
        pts = (corners @ M[:2, :2].T + M[:2, 2]) / w[..., None]
    new = np.concatenate([pts.min(1), pts.max(1)], axis=1).reshape(-1, 4)
    new = np.clip(new, 0, S)
    w1, h1 = (b[:, 2] - b[:, 0]) * scale, (b[:, 3] - b[:, 1]) * scale
    w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
    eps = 1e-16
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    keep = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + eps) > 0.1) & (ar < 100)
    new, lab = new[keep], labels[keep]
    if flip:
        new = np.stack([S - new[:, 2], new[:, 1], S - new[:, 0], new[:, 3]], axis=1)
    if flipud:
        new = np.stack([new[:, 0], S - new[:, 3], new[:, 2], S - new[:, 1]], axis=1)
    return new.astype(np.float32), lab.astype(np.int32)


class DetAugment:
    """Draws one record per output image.  Seeded from Python's `random` unless a seed is given.  The names and defaults
    are the trainer's; a knob at 0 draws nothing, so the default stream is independent of the non-default knobs."""

    def __init__(self, size: int, seed: Optional[int] = None, mosaic: float = 1.0, hsv=(0.015, 0.7, 0.4),
                 fliplr: float = 0.5, translate: float = 0.1, scale: float = 0.5, degrees: float = 0.0, shear: float = 0.0,
                 perspective: float = 0.0, flipud: float = 0.0, mixup: float = 0.0):
        for name, v, lo, hi, closed in (("degrees", degrees, 0, 180, True), ("shear", shear, 0, 89, False),
                                        ("perspective", perspective, 0, 0.001, True), ("flipud", flipud, 0, 1, True),
                                        ("mixup", mixup, 0, 1, True), ("fliplr", fliplr, 0, 1, True), ("mosaic", mosaic, 0, 1, True)):
            if not (lo <= v <= hi if closed else lo <= v < hi):                      # also rejects NaN
                raise YvError(f"DetAugment: {name}={v} is outside [{lo}, {hi}{']' if closed else ')'}")
        self.S = int(size)
        self.rng = np.random.default_rng(random.getrandbits(63) if seed is None else seed)
        self.mosaic, self.hsv, self.fliplr, self.translate, self.scale = mosaic, hsv, fliplr, translate, scale
        self.degrees, self.shear, self.perspective, self.flipud, self.mixup = degrees, shear, perspective, flipud, mixup

    def _geometry(self, index: int, n_dataset: int, use_mosaic: bool) -> dict:
        """Mosaic sources and centre, then the draws of RandomPerspective.affine_transform in the published order:
        perspective, angle, scale, shear, translate."""
        S, r = self.S, self.rng
        mosaic = bool(use_mosaic and r.random() < self.mosaic)
        p = dict(mosaic=mosaic, sources=[index])
        if mosaic:
            p["sources"] += [int(v) for v in r.integers(0, n_dataset, 3)]
            p["centre"] = (int(r.uniform(S / 2, 3 * S / 2)), int(r.uniform(S / 2, 3 * S / 2)))       # (xc, yc)
        if self.perspective:
            p["perspective"] = (float(r.uniform(-self.perspective, self.perspective)),
                                float(r.uniform(-self.perspective, self.perspective)))
        if self.degrees:
            p["angle"] = float(r.uniform(-self.degrees, self.degrees))
        p["scale"] = float(r.uniform(1 - self.scale, 1 + self.scale))
        if self.shear:
            p["shear"] = (float(r.uniform(-self.shear, self.shear)), float(r.uniform(-self.shear, self.shear)))
        p["translate"] = (float(r.uniform(0.5 - self.translate, 0.5 + self.translate)),
                          float(r.uniform(0.5 - self.translate, 0.5 + self.translate)))
        return p

    def plan(self, index: int, n_dataset: int, use_mosaic: bool = True) -> dict:
        r = self.rng
        p = self._geometry(index, n_dataset, use_mosaic)
        if use_mosaic and self.mixup and r.random() < self.mixup:        # MixUp: a second image with a geometry of its own
            p["mix"] = self._geometry(int(r.integers(0, n_dataset)), n_dataset, use_mosaic)
            p["mix_ratio"] = float(r.beta(32.0, 32.0))
        if self.flipud:
            p["flipud"] = bool(r.random() < self.flipud)
        p["hsv"] = [float(v) for v in r.uniform(-1, 1, 3) * np.asarray(self.hsv) + 1]
        p["flip"] = bool(r.random() < self.fliplr)
        return p


def plan_layers(plan: dict) -> List[dict]:
    """The geometric plans of one output image: the plan itself and, under MixUp, its `mix` entry."""
    return [plan, plan["mix"]] if plan.get("mix") else [plan]


def plan_is_default(plan: dict) -> bool:
    """True when `yv_mosaic_augment` can produce the image: no rotation, shear, perspective, vertical flip or second layer."""
    return (not plan.get("mix") and not plan.get("flipud") and plan.get("angle", 0.0) == 0
            and tuple(plan.get("shear", (0, 0))) == (0, 0) and tuple(plan.get("perspective", (0, 0))) == (0, 0))


def _placement(layer: dict, sizes: Sequence[Tuple[int, int]], tile_ids: Sequence[int], S: int):
    """Placement rectangles of one geometric plan -> rec_i (34) i32 with the flip word 0, label offsets, canvas size."""
    rec_i = np.zeros(34, dtype=np.int32)
    offs = []
    if layer["mosaic"]:
        canvas = 2 * S
        xc, yc = layer["centre"]
        for i, ((w, h), tid) in enumerate(zip(sizes, tile_ids)):
            (x1a, y1a, x2a, y2a), (x1b, y1b) = mosaic_placement(i, xc, yc, w, h, S)
            rec_i[2 + 8 * i:2 + 8 * i + 7] = (tid, x1a, y1a, x2a, y2a, x1b, y1b)
            offs.append((x1a - x1b, y1a - y1b))
        rec_i[0] = 4
    else:
        canvas = S
        (w, h), tid = sizes[0], tile_ids[0]
        left, top = int(round((S - w) / 2 - 0.1)), int(round((S - h) / 2 - 0.1))                         # LetterBox(center)
        rec_i[2:9] = (tid, left, top, left + w, top + h, 0, 0)
        offs.append((left, top))
        rec_i[0] = 1
    return rec_i, offs, canvas


def build_record(plan: dict, sizes: Sequence[Tuple[int, int]], tile_ids: Sequence[int], S: int):
    """plan + resized source sizes [(w,h)] + their tile slots -> rec_f (6) f32, rec_i (34) i32, lut (3,256) u8, the forward
    matrix and the per-source label offsets (padw, padh) on the canvas.  The record of `yv_mosaic_augment`: scale,
    translate, HSV and the horizontal flip only (`build_record_ex` carries the rest)."""
    rec_i, offs, canvas = _placement(plan, sizes, tile_ids, S)
    rec_i[1] = int(plan["flip"])
    M = affine_matrix(canvas, S, plan["scale"], *plan["translate"])
    rec_f = np.linalg.inv(M)[:2].reshape(-1).astype(np.float32)
    return rec_f, rec_i, hsv_tables(plan["hsv"]), M, offs, canvas


def build_record_ex(plan: dict, sizes: Sequence[Sequence[Tuple[int, int]]], tile_ids: Sequence[Sequence[int]], S: int):
    """The record of `yv_mosaic_augment_ex`.  `sizes` and `tile_ids` hold one list per layer of `plan_layers(plan)`.
    -> rec_h (layers,9) f32, rec_i (layers,34) i32, mix weight of layer 0 (1.0 without MixUp), lut (3,256) u8, and per
    layer the forward matrix, the label offsets and the canvas size.  Flip word (layer 0): bit 0 fliplr, bit 1 flipud."""
    layers = plan_layers(plan)
    rec_h, rec_i = np.zeros((len(layers), 9), np.float32), np.zeros((len(layers), 34), np.int32)
    Ms, offs, canvases = [], [], []
    for k, (layer, sz, ids) in enumerate(zip(layers, sizes, tile_ids)):
        rec_i[k], o, cv = _placement(layer, sz, ids, S)
        M = layer_matrix(layer, cv, S)
        rec_h[k] = homography_record(M)
        Ms.append(M); offs.append(o); canvases.append(cv)
    rec_i[0, 1] = int(bool(plan["flip"])) | (int(bool(plan.get("flipud", False))) << 1)
    mix = float(plan["mix_ratio"]) if len(layers) == 2 else 1.0
    return rec_h, rec_i, mix, hsv_tables(plan["hsv"]), Ms, offs, canvases


def batch_records_ex(plans: Sequence[dict], sizes: dict, slot: dict, S: int):
    """The arguments of one `mosaic_augment_ex` call.  sizes: source -> (w,h) of its tile, slot: source -> tile index.
    Two layers as soon as one image mixes; an image that does not mix then carries mix = 1 and a copy of its own record as
    layer 1.  -> rec_h (B,L,9) f32, rec_i (B,L,34) i32, mix (B) f32, lut (B,3,256) u8."""
    B, L = len(plans), 2 if any(p.get("mix") for p in plans) else 1
    rec_h, rec_i = np.zeros((B, L, 9), np.float32), np.zeros((B, L, 34), np.int32)
    mix, lut = np.ones((B,), np.float32), np.zeros((B, 3, 256), np.uint8)
    for b, p in enumerate(plans):
        layers = plan_layers(p)
        h, i, mix[b], lut[b], _, _, _ = build_record_ex(p, [[sizes[s] for s in l["sources"]] for l in layers],
                                                        [[slot[s] for s in l["sources"]] for l in layers], S)
        rec_h[b, :len(layers)], rec_i[b, :len(layers)] = h, i
        if len(layers) < L:
            rec_h[b, 1], rec_i[b, 1] = h[0], i[0]
    return rec_h, rec_i, mix, lut


def plan_labels(plan: dict, labs: dict, sizes: dict, S: int):
    """Labels of one output image, on the host alone.  labs: source -> (n,5) rows {class, xc, yc, w, h} (normalised, as the
    YOLO txt files), sizes: source -> (w,h) of the resized tile.  Every layer's boxes go to its canvas, through its own
    forward matrix and the shared flips; MixUp concatenates the layers.  -> boxes (n,4) f32 xyxy, labels (n) i32."""
    out_b, out_l = [], []
    for layer in plan_layers(plan):
        srcs = layer["sources"]
        _, offs, cv = _placement(layer, [sizes[s] for s in srcs], [0] * len(srcs), S)
        M = layer_matrix(layer, cv, S)
        bb, ll = [], []
        for s, (px, py) in zip(srcs, offs):
            lab, (w, h) = labs[s], sizes[s]
            if len(lab):
                xy = np.stack([(lab[:, 1] - lab[:, 3] / 2) * w + px, (lab[:, 2] - lab[:, 4] / 2) * h + py,
                               (lab[:, 1] + lab[:, 3] / 2) * w + px, (lab[:, 2] + lab[:, 4] / 2) * h + py], axis=1)
                bb.append(xy); ll.append(lab[:, 0])
        if bb:
            xy, lb = np.clip(np.concatenate(bb), 0, cv), np.concatenate(ll)
            good = (xy[:, 2] > xy[:, 0]) & (xy[:, 3] > xy[:, 1])                     # boxes clipped away by the canvas
            nb, nl = transform_boxes(xy[good], lb[good], M, layer["scale"], S, plan["flip"], bool(plan.get("flipud", False)))
            out_b.append(nb); out_l.append(nl)
    if not out_b:
        return np.zeros((0, 4), np.float32), np.zeros((0,), np.int32)
    return np.concatenate(out_b), np.concatenate(out_l)


def augment_batch(samples: List[Tuple[str, str]], batch_idx: Sequence[int], aug: DetAugment, max_boxes: int, device: str,
                  use_mosaic: bool = True):
    """One training batch: decodes the planned sources, resizes them into tiles and composes the outputs on the device:
    one `mosaic_augment` launch while every plan is free of the non-default features, else one `mosaic_augment_ex` launch
    (two layers as soon as one image mixes; the others carry mix = 1 and a copy of their own record as layer 1).
    -> images (B,S,S,3) u8 cuda, gt boxes (B,G,4) f32, gt labels (B,G) i32, counts (B) i32 (host tensors)."""
    import torch
    from PIL import Image
    import yvhip
    from . import letterbox
    from .yolo_data import parse_label_text
    S, B = aug.S, len(batch_idx)
    plans = [aug.plan(int(i), len(samples), use_mosaic) for i in batch_idx]
    src_ids = sorted({s for p in plans for layer in plan_layers(p) for s in layer["sources"]})
    slot = {s: k for k, s in enumerate(src_ids)}
    ims = [np.asarray(Image.open(samples[s][0]).convert("RGB")) for s in src_ids]
    Hc, Wc = max(im.shape[0] for im in ims), max(im.shape[1] for im in ims)
    canvas = np.zeros((len(ims), Hc, Wc, 3), dtype=np.uint8)
    geom = np.zeros((len(ims), 6), dtype=np.int32)
    sizes, labs = {}, {}
    for k, (s, im) in enumerate(zip(src_ids, ims)):
        h0, w0 = im.shape[:2]
        canvas[k, :h0, :w0] = im
        nw, nh = tile_geometry(w0, h0, S)
        geom[k] = (w0, h0, nw, nh, 0, 0)
        sizes[s] = (nw, nh)
        lp = samples[s][1]
        labs[s] = parse_label_text(open(lp).read()) if os.path.exists(lp) else np.zeros((0, 5))
    tiles = letterbox(torch.from_numpy(canvas).to(device), torch.from_numpy(geom).to(device), S)
    boxes = np.zeros((B, max_boxes, 4), dtype=np.float32)
    labels = np.zeros((B, max_boxes), dtype=np.int32)
    counts = np.zeros((B,), dtype=np.int32)
    for b, p in enumerate(plans):
        nb, nl = plan_labels(p, labs, sizes, S)
        n = min(len(nb), max_boxes)
        boxes[b, :n], labels[b, :n], counts[b] = nb[:n], nl[:n], n
    if all(plan_is_default(p) for p in plans):
        rec_f, rec_i, lut = np.zeros((B, 6), np.float32), np.zeros((B, 34), np.int32), np.zeros((B, 3, 256), np.uint8)
        for b, p in enumerate(plans):
            srcs = p["sources"]
            rec_f[b], rec_i[b], lut[b], _, _, _ = build_record(p, [sizes[s] for s in srcs], [slot[s] for s in srcs], S)
        out = yvhip.mosaic_augment(tiles, torch.from_numpy(rec_f).to(device), torch.from_numpy(rec_i).to(device),
                                   torch.from_numpy(lut).to(device))
    else:
        rec_h, rec_i, mix, lut = batch_records_ex(plans, sizes, slot, S)
        out = yvhip.mosaic_augment_ex(tiles, torch.from_numpy(rec_h).to(device), torch.from_numpy(rec_i).to(device),
                                      torch.from_numpy(mix).to(device) if rec_h.shape[1] == 2 else None, torch.from_numpy(lut).to(device))
    return out, torch.from_numpy(boxes), torch.from_numpy(labels), torch.from_numpy(counts)
