"""`main` / `draw_image` of the missing `YOLOTensorRT.inferdet` (app.py:16,61,77; test.py:28), rebuilt
batch-first on the device pipeline.  Reconstructed from the sibling walkthrough
(YOLOTensorRT_yolodet_py_解读.md:33-116) and the callers' keyword arguments; semantics the tree cannot pin
are defined here and listed in DESIGN.md (ensemble = mean of logits; crops are RGB; the reported `sort` is
the classifier's class).
"""
import os
import threading
from typing import Callable, List, Optional

import numpy as np
import torch

import yvhip
from yvhip.engines import _env_flag
from yvhip.pipeline import DetectClassifyPipeline

from .config import CLASSES, COLORS
from .models.utils import letterbox_geometry, path_to_list, rect_net_shape

BATCH = 32


def draw_image(image, box, cls):
    """Rectangle + "{CLASS}:1" label (解读.md:35-45) with PIL (OpenCV is not required)."""
    from PIL import Image, ImageDraw
    arr = np.asarray(image)
    im = Image.fromarray(arr[..., ::-1].copy())               # callers hand over BGR
    d = ImageDraw.Draw(im)
    color = COLORS[int(cls) % len(COLORS)][::-1]
    x0, y0, x1, y1 = [int(v) for v in box]
    d.rectangle([x0, y0, x1, y1], outline=color, width=2)
    d.text((x0, max(0, y0 - 12)), f"{CLASSES[int(cls)]}:1", fill=color)
    return np.asarray(im)[..., ::-1].copy()


def _load_rgb(path: str) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _pipeline(Engine, det, model_list, fit_crops: bool = False) -> DetectClassifyPipeline:
    vits = [m.engine() for m in model_list]
    return DetectClassifyPipeline(det, vits, Engine.score_threshold, Engine.iou_threshold, Engine.topk,
                                  fit_crops=fit_crops)


def _detector(Engine, small_maps: Optional[bool], grouped_head: Optional[bool] = None):
    """Engine.engine, or - where small_maps or grouped_head is given and differs from its flag - its sibling in that state (shared
    weights, own buffers), built once per Engine and state and kept on it: later calls reuse its activation buffers."""
    det = Engine.engine
    want = (det.small_maps if small_maps is None else bool(small_maps),
            det.grouped_head if grouped_head is None else bool(grouped_head))
    if want == (det.small_maps, det.grouped_head):
        return det
    cache = Engine.__dict__.setdefault("_detector_siblings", {})
    sib = cache.get(want)
    if sib is None or sib.w is not det.w or sib.hw != det.hw:
        sib = cache[want] = det.resized(det.size)
        sib.small_maps, sib.grouped_head = want
    return sib


def _rect_pipeline(Engine, pipe: DetectClassifyPipeline, cache: dict, hw) -> DetectClassifyPipeline:
    """`pipe` with the detector resized to `hw` (shared weights, own buffers); one per shape."""
    if hw not in cache:
        cache[hw] = DetectClassifyPipeline(pipe.yolo.resized(hw), pipe.vits, Engine.score_threshold, Engine.iou_threshold,
                                           Engine.topk, fit_crops=pipe.fit_crops)
    return cache[hw]


def run_chunk(run: DetectClassifyPipeline, arrs: List[np.ndarray], new_shape, net, dev):
    """One chunk of main on the eager pipeline, host arrays in to host reads out: canvas + geometry upload, letterbox into `net`
    (new_shape is its (W, H)), the pipeline call, the reads.  -> (det_count list, det_box, det_score, det_label, cls_of) with
    cls_of {(image, slot): class} of the classified crops.  (What RequestSession.run does in one upload, two graph replays and
    one download; tools/request_bench.py times the two against each other.)"""
    B = len(arrs)
    Hc, Wc = max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs)
    canvas = np.zeros((B, Hc, Wc, 3), dtype=np.uint8)
    geom, ratio, dwdh, wh = [], [], [], []
    for i, a in enumerate(arrs):
        h, w = a.shape[:2]
        canvas[i, :h, :w] = a
        r, (dw, dh), (nw, nh), (left, top) = letterbox_geometry(h, w, new_shape)
        geom.append([w, h, nw, nh, left, top]); ratio.append(r); dwdh += [dw, dh]; wh += [w, h]
    src = torch.from_numpy(canvas).to(dev)
    net_in = yvhip.letterbox(src, torch.tensor(geom, dtype=torch.int32, device=dev), net)
    out = run(net_in, torch.tensor(ratio, dtype=torch.float32, device=dev),
              torch.tensor(dwdh, dtype=torch.float32, device=dev), torch.tensor(wh, dtype=torch.int32, device=dev),
              src_images=src)
    cnt = out["det_count"].cpu().tolist()
    box, score, dlab = out["det_box"].cpu(), out["det_score"].cpu(), out["det_label"].cpu()
    clist, ctot, clab = out["crop_list"].cpu(), int(out["crop_total"][0]), out["cls_label"].cpu()
    cls_of = {(int(clist[k, 0]), int(clist[k, 5])): int(clab[k]) for k in range(ctot)}
    return cnt, box, score, dlab, cls_of


def _object(c: int, dlab: int, score: float, box) -> dict:
    x0, y0, x1, y1 = box
    return {"sort": CLASSES[c], "det_sort": CLASSES[dlab % len(CLASSES)], "confidence": score,
            "xmin": x0, "ymin": y0, "xmax": x1, "ymax": y1}


def _objects_of_reads(cnt, box, score, dlab, cls_of) -> List[list]:
    """The objects of each image of a chunk from run_chunk's reads: its detections with a classified crop, in score order."""
    per_image = []
    for i in range(len(cnt)):
        objs = []
        for k in range(cnt[i]):
            c = cls_of.get((i, k))
            if c is None:                           # degenerate crop: the reference's PIL crop would raise
                continue
            objs.append(_object(c, int(dlab[i, k]), float(score[i, k]), box[i, k].tolist()))
        per_image.append(objs)
    return per_image


def _objects_of_records(rec: dict, B: int) -> List[list]:
    """The same from a RequestSession's records: they are the classified crops, image ascending, then score order."""
    per_image = [[] for _ in range(B)]
    for k in range(len(rec["image"])):
        per_image[int(rec["image"][k])].append(_object(int(rec["cls_label"][k]), int(rec["det_label"][k]), float(rec["score"][k]),
                                                       rec["box"][k].tolist()))
    return per_image


SESSIONS_PER_ENGINE = 4
_SESSION_LOCK = threading.Lock()


def _session(Engine, det, pipe: DetectClassifyPipeline, model_list):
    """The RequestSession of this Engine for the detector `det` and the classifier modules of model_list, kept on Engine like
    _detector_siblings: one per (state of the detector's small_maps / grouped_head flags, identities of the modules), so requests
    that alternate between classifier lists each keep their captures; SESSIONS_PER_ENGINE are kept, least recently used first
    out.  The entry is valid while its engines ARE pipe's objects and pipe would freeze what the session froze
    (RequestSession.matches): a retrained module builds a new engine, a changed threshold another launch - the entry is then
    dropped and built again under the same key.  Found and built under one lock, so two first requests build one session.
    Every session of an Engine shares one stream - a stream's first launch registers a 64 MB workspace that stays with its
    handle - and therefore one lock."""
    from collections import OrderedDict
    from yvhip.request import RequestSession
    key = (det.small_maps, det.grouped_head, tuple(id(m) for m in model_list))
    with _SESSION_LOCK:
        cache = Engine.__dict__.setdefault("_request_sessions", OrderedDict())
        shared = Engine.__dict__.setdefault("_request_shared", {})
        if not shared:
            shared.update(stream=torch.cuda.Stream(device=det.dev), lock=threading.Lock())
        ses = cache.get(key)
        if ses is None or not ses.matches(pipe):
            ses = cache[key] = RequestSession(pipe, stream=shared["stream"], lock=shared["lock"])
        cache.move_to_end(key)
        while len(cache) > SESSIONS_PER_ENGINE:
            cache.popitem(last=False)
    return ses


def main(Engine, imgs, device=None, model_list: Optional[list] = None, transform=None, aliyunoss=None,
         func: Optional[Callable] = None, rect: bool = False, fit_crops: Optional[bool] = None,
         small_maps: Optional[bool] = None, grouped_head: Optional[bool] = None, graph: Optional[bool] = None):
    """Detect + classify every image under `imgs` (directory, file or list).  Returns a JSON-serialisable dict
    {"output": [{"image": name, "objects": [{"sort", "det_sort", "confidence", "xmin", "ymin", "xmax", "ymax"}]}]}.
    `transform` is accepted for signature compatibility: its valid_test branch (nearest resize to 224 +
    Normalize(.5,.5)) is what the fused crop kernel implements.  `func(folder, filename, path, objects)` is
    called per image like test.py:28 does with generate_annotation.
    rect=True: each chunk of images is letterboxed into the smallest stride-32 rectangle that holds it at the engine's size
    (models.utils.rect_net_shape; the engine must be square) instead of the S x S square, and the detector runs at that
    extent (YoloEngine.resized, one engine per shape).  Restored coordinates, crops and the result layout are the same.
    fit_crops=True (None: the environment variable YV_FIT_CROPS, "1" = on): the classifier of each chunk is sized to the crops
    the detector found instead of topk per image (DetectClassifyPipeline(fit_crops=True)): for request-sized calls.  The result
    is the same dict; classifiers built with mid_gemm=True use their mid-M GEMM, main does not switch it on.
    small_maps (None: as the engine was built): the detector of this call runs with YoloEngine(small_maps=) in that state - where
    it differs from Engine.engine's, on a sibling that shares its weights (YoloEngine.resized), built once and kept on Engine.
    grouped_head (None: as the engine was built): likewise for YoloEngine(grouped_head=); one sibling per pair of the two flags.
    graph=True (None: the environment variable YV_REQUEST_GRAPH, "1" = on): each chunk goes through a yvhip.request.RequestSession
    kept on Engine - one upload, two captured-graph replays (detect stage, classifier fitted to the crops) and one download of
    packed records - in place of the eager calls and their eleven small copies.  The result is the same dict; fit_crops is
    implied.  A chunk shape seen for the first time is captured then (seconds); with rect=True: YvError, a session has one
    detector extent."""
    graph = _env_flag(graph, "YV_REQUEST_GRAPH")
    if graph and rect:
        raise yvhip.YvError("graph=True does not take rect=True: a request session replays one detector extent")
    yvhip.require_gpu()
    if not model_list:
        raise yvhip.YvError("model_list is empty")
    dev = torch.device(device) if device is not None else Engine.device
    S = Engine.size
    det = _detector(Engine, small_maps, grouped_head)
    pipe = _pipeline(Engine, det, model_list, _env_flag(fit_crops, "YV_FIT_CROPS") or graph)
    session = _session(Engine, det, pipe, model_list) if graph else None
    if rect and not isinstance(S, int):
        raise yvhip.YvError("rect=True takes a square engine: its size is the long side of every rectangle")
    rect_pipes: dict = {}
    paths = path_to_list(imgs)
    results = []
    for s in range(0, len(paths), BATCH):
        chunk = paths[s:s + BATCH]
        arrs = [_load_rgb(p) for p in chunk]
        if session is not None:
            per_image = _objects_of_records(session.run(arrs), len(arrs))
        elif rect:
            Hn, Wn = rect_net_shape([a.shape[:2] for a in arrs], S)
            per_image = _objects_of_reads(*run_chunk(_rect_pipeline(Engine, pipe, rect_pipes, (Hn, Wn)), arrs, (Wn, Hn), (Hn, Wn), dev))
        else:
            per_image = _objects_of_reads(*run_chunk(pipe, arrs, (S, S), S, dev))
        for i, p in enumerate(chunk):
            objs = per_image[i]
            name = os.path.basename(p)
            if func is not None:
                func(os.path.basename(os.path.dirname(p)) or "image", name, p, objs)
            if aliyunoss is not None and hasattr(aliyunoss, "put_object_from_file"):
                aliyunoss.put_object_from_file(name, p)
            results.append({"image": name, "objects": objs})
    results.sort(key=lambda r: r["image"])
    return {"output": results}
