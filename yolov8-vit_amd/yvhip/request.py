"""Request sessions: a request-sized call (inferdet.main on a few images) as one upload, two graph replays and one download.

A DetectClassifyPipeline call at request size is bound by the host's enqueue: about 140 launches of kernels that mostly run
7-20 us (DESIGN.md sections 31, 32, 37).  The whole step has no host synchronisation, so it replays from a captured graph
(tests/test_gpu_models.py::test_step_is_graph_capturable); with fit_crops the crop count is read on the host between the two
stages, so a session keeps TWO graphs per shape:

  stage 1   letterbox -> detector -> efficient_nms -> postprocess_dets -> compact_crops      key (B, Hc, Wc)
  stage 2   crop_resize_norm -> backbone(s) -> head(s) -> pack_results                       key (B, Hc, Wc, capacity)

Hc, Wc are the chunk's largest height and width rounded up to multiples of 64 (session_key), capacity is
fit_capacity(crops, cap).  The request's geometry travels as ONE block of 32-bit words (request_block) whose device copy the
kernels read through views; the result comes back as ONE buffer of records (yv_pack_results, unpack_results).
"""
from __future__ import annotations

import collections
import contextlib
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import YvError

RECORD_FIELDS = 9                   # image, slot, box x 4, det_label, cls_label, score; the class logits follow
KEY_ROUND = 64                      # canvas sides of a stage-1 key are multiples of this


def session_key(B: int, h_max: int, w_max: int) -> Tuple[int, int, int]:
    """Stage-1 key of a chunk of B images whose largest height / width are h_max / w_max: (B, Hc, Wc), the sides rounded up to
    multiples of 64."""
    if B <= 0 or h_max <= 0 or w_max <= 0:
        raise YvError("session_key: B, h_max and w_max must be positive")
    up = lambda v: (int(v) + KEY_ROUND - 1) // KEY_ROUND * KEY_ROUND
    return int(B), up(h_max), up(w_max)


def block_layout(B: int) -> Dict[str, Tuple[int, int]]:
    """Word ranges (start, stop) of the request block of B images: {geom (B, 6) i32 | ratio (B) f32 | dwdh (2B) f32 | wh (2B)
    i32}; "words" is its length, 11 B."""
    return {"geom": (0, 6 * B), "ratio": (6 * B, 7 * B), "dwdh": (7 * B, 9 * B), "wh": (9 * B, 11 * B), "words": (0, 11 * B)}


def request_block(shapes: Sequence[Tuple[int, int]], new_shape: Tuple[int, int], out: Optional[np.ndarray] = None) -> np.ndarray:
    """The request block of images of `shapes` ((h, w) pairs) letterboxed into new_shape = (W, H): the host arithmetic of
    inferdet.main (letterbox_geometry), floats stored by their bits.  out: an int32 array of 11 B words to fill."""
    from YOLOTensorRT.models.utils import letterbox_geometry
    B = len(shapes)
    lay = block_layout(B)
    blk = np.empty(lay["words"][1], dtype=np.int32) if out is None else out
    if blk.dtype != np.int32 or blk.shape != (lay["words"][1],):
        raise YvError("request_block: out must be an int32 array of 11 B words")
    geom, f = blk[slice(*lay["geom"])].reshape(B, 6), blk.view(np.float32)
    ratio, dwdh, wh = f[slice(*lay["ratio"])], f[slice(*lay["dwdh"])].reshape(B, 2), blk[slice(*lay["wh"])].reshape(B, 2)
    for i, (h, w) in enumerate(shapes):
        r, (dw, dh), (nw, nh), (left, top) = letterbox_geometry(h, w, new_shape)
        geom[i] = (w, h, nw, nh, left, top)
        ratio[i], dwdh[i], wh[i] = r, (dw, dh), (w, h)
    return blk


def unpack_results(words: np.ndarray, nc: int) -> Dict[str, np.ndarray]:
    """words: the (1 + cap, 9 + nc) int32 buffer of yv_pack_results (or its first rows: at least 1 + total) -> numpy arrays of
    the `total` records: image, slot, box (n, 4), det_label, cls_label (int32), score (n) f32, logits (n, nc) f32."""
    words = np.asarray(words)
    W = RECORD_FIELDS + int(nc)
    if words.dtype != np.int32 or words.ndim != 2 or words.shape[1] != W or words.shape[0] < 1:
        raise YvError(f"unpack_results: expected (1 + cap, {W}) int32 words")
    n = int(words[0, 0])
    if int(words[0, 4]) != nc or n < 0 or n > words.shape[0] - 1:
        raise YvError("unpack_results: the header does not describe this buffer")
    rows = words[1:1 + n].copy()                         # the caller's buffer is a session's pinned download area: own every array
    return dict(image=rows[:, 0].copy(), slot=rows[:, 1].copy(), box=rows[:, 2:6].copy(), det_label=rows[:, 6].copy(),
                cls_label=rows[:, 7].copy(), score=rows[:, 8].copy().view(np.float32),
                logits=rows[:, 9:].copy().view(np.float32).reshape(n, nc))


def empty_results(nc: int) -> Dict[str, np.ndarray]:
    head = np.zeros((1, RECORD_FIELDS + nc), dtype=np.int32)
    head[0, 4] = nc
    return unpack_results(head, nc)


def check_images(arrs) -> List[np.ndarray]:
    """The images of a request: a non-empty list of (h, w, 3) uint8 arrays with h, w > 0; anything else is a YvError."""
    if not isinstance(arrs, (list, tuple)) or len(arrs) == 0:
        raise YvError("a request takes a non-empty list of (h, w, 3) uint8 RGB arrays")
    for a in arrs:
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] <= 0 or a.shape[1] <= 0:
            raise YvError("a request takes (h, w, 3) uint8 RGB arrays")
    return list(arrs)


PIPE_FROZEN = ("score_threshold", "iou_threshold", "topk", "conf", "dedupe_iou", "coord_mode", "max_crops", "capacity", "parts")
YOLO_FROZEN = ("hw", "dtype", "small_maps", "grouped_head", "dma32", "fused_c2f", "fused_tail")
VIT_FROZEN = ("dtype", "img", "cls_tail", "fused_ln", "long_attn", "mid_gemm", "ln_gemm", "full_cus_from")


def frozen_state(pipe) -> tuple:
    """What a capture of `pipe`'s stages freezes besides the engines themselves: the pipeline's thresholds and sizes and the
    engine attributes its launch lists read.  A session whose pipeline no longer gives this tuple captures again."""
    return (tuple(getattr(pipe, a) for a in PIPE_FROZEN), tuple(getattr(pipe.yolo, a) for a in YOLO_FROZEN),
            tuple(tuple(getattr(v, a) for a in VIT_FROZEN) for v in pipe.vits))


class _Stage2:
    """One captured classifier stage: its graph, the tensors it wrote and the pinned copy of its records."""

    def __init__(self):
        self.graph, self.out, self.packed, self.host, self.bufs = None, None, None, None, None


class _Key:
    """What a stage-1 key owns: canvases, request block, graph, the detect stage's outputs, its stage-2 graphs."""

    def __init__(self, key, dev):
        B, Hc, Wc = key
        self.key = key
        self.canvas_host = torch.zeros((B, Hc, Wc, 3), dtype=torch.uint8).pin_memory()
        self.canvas = torch.zeros((B, Hc, Wc, 3), dtype=torch.uint8, device=dev)
        lay = block_layout(B)
        self.block_host = torch.zeros((lay["words"][1],), dtype=torch.int32).pin_memory()
        self.block = torch.zeros((lay["words"][1],), dtype=torch.int32, device=dev)
        blk, f = self.block, self.block.view(torch.float32)               # the kernels read views of the device copy
        self.geom, self.ratio = blk[slice(*lay["geom"])].view(B, 6), f[slice(*lay["ratio"])]
        self.dwdh, self.wh = f[slice(*lay["dwdh"])], blk[slice(*lay["wh"])]
        self.total_host = torch.zeros((1,), dtype=torch.int32).pin_memory()
        self.graph, self.det, self.bufs = None, None, None
        self.stage2: Dict[int, _Stage2] = {}


class RequestSession:
    """session.run(arrs): list of (h, w, 3) u8 RGB arrays of any sizes -> the records of unpack_results, equal to what
    DetectClassifyPipeline(fit_crops=True) gives on the same images.

    pipe: a DetectClassifyPipeline; the session always fits the classifier to the crops, whatever pipe.fit_crops says.  Each
    stage of a key runs once eagerly on the session's stream at its first visit (workspace registration, the engines' buffer
    sets of that size), is then captured on that one stream, and every result - the first included - comes from a replay.  The
    options an engine sets around its pass (mid_gemm, small_maps, grouped_head, ...) are decided at capture, as for any launch.
    A replay runs inside the guards the eager stages take (yolo.guard, v.guard(0)), so StepGuard orders it against an eager user
    of the same engines; the session keeps references to the engines, their buffer sets and every tensor a graph reads or writes.
    Pixels outside an image's w x h corner of the canvas are never read (letterbox_kernel clamps to w - 1, h - 1; the crop
    rectangles are clamped to img_wh), so the host writes the corners only and clears nothing.
    max_keys stage-1 keys are kept, least recently used first out; evicting one drops its graphs, static buffers and stage-2
    graphs.  `stats` counts eager stage runs, captures, replays and evictions.  run() is serialised by a lock.
    A capture freezes frozen_state(pipe); run() and warm() compare it and, where an attribute was flipped since, drop every key
    (counted as evictions) and capture again.  The returned arrays are the caller's: none aliases a session buffer.
    stream, lock: sessions that share one stream (its first launch registers a 64 MB split-K workspace that is kept for the
    stream's handle) must share one lock, since a capture owns the stream; default: a stream and a lock of the session's own.
    A first visit is not cheap for a serving process: torch.cuda.graph collects garbage, synchronises the DEVICE and empties
    the allocator's cache on entry, so other threads' GPU work waits for it; warm() does it ahead of the first request."""

    def __init__(self, pipe, max_keys: int = 8, stream: Optional["torch.cuda.Stream"] = None, lock=None):
        from . import require_gpu
        require_gpu()
        if max_keys < 1:
            raise YvError("max_keys must be at least 1")
        self.pipe, self.max_keys = pipe, int(max_keys)
        self.yolo, self.vits = pipe.yolo, list(pipe.vits)
        self.dev = self.yolo.dev
        self.nc = self.vits[0].nc
        self.stream = torch.cuda.Stream(device=self.dev) if stream is None else stream
        self.frozen = frozen_state(pipe)
        self.keys: "collections.OrderedDict[tuple, _Key]" = collections.OrderedDict()
        self.stats = {"eager": 0, "captures": 0, "replays": 0, "evictions": 0}
        self.last = {}                                   # of the last run: its keys (tools, tests)
        self._lock = threading.Lock() if lock is None else lock

    # ---------------------------------------------------------------------------------------------------- keys
    def _net(self):
        H, W = self.yolo.hw
        return (W, H), self.yolo.size

    def _refreeze(self):
        """An attribute a capture froze was flipped: every key is stale."""
        now = frozen_state(self.pipe)
        if now != self.frozen:
            self.stats["evictions"] += len(self.keys)
            self.keys.clear()
            self.frozen = now

    def _key(self, key) -> _Key:
        k = self.keys.get(key)
        if k is not None:
            self.keys.move_to_end(key)
            return k
        while len(self.keys) >= self.max_keys:
            self.keys.popitem(last=False)                # every run ends synchronised: nothing of it is in flight
            self.stats["evictions"] += 1
        k = self.keys[key] = _Key(key, self.dev)
        return k

    # ---------------------------------------------------------------------------------------------------- stages
    def _stage1(self, k: _Key) -> dict:
        from . import letterbox
        net_in = letterbox(k.canvas, k.geom, self._net()[1])
        return self.pipe.detect_stage(net_in, k.ratio, k.dwdh, k.wh)

    def _stage2(self, k: _Key, capacity: int):
        from . import pack_results
        det = dict(k.det)
        det["capacity"] = capacity
        out = self.pipe.classify_stage(k.canvas, det)
        return out, pack_results(out, out["cls_label"], out["cls_logits"], capacity)

    def _vit_guards(self) -> contextlib.ExitStack:
        st = contextlib.ExitStack()
        for v in self.vits:
            st.enter_context(v.guard(0))
        return st

    def _captured(self, fn):
        """fn once eagerly, then captured: (graph, what fn returned under capture)."""
        fn()
        self.stats["eager"] += 1
        self.stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        # thread_local: another request thread's eager HIP calls (an allocation, a copy) do not invalidate this capture
        with torch.cuda.graph(graph, stream=self.stream, capture_error_mode="thread_local"):
            res = fn()
        self.stats["captures"] += 1
        return graph, res

    def _detect(self, k: _Key) -> int:
        """Stage 1 of key k on the uploaded request: the crop count."""
        with self.yolo.guard:
            if k.graph is None:
                k.graph, k.det = self._captured(lambda: self._stage1(k))
                k.bufs = self.yolo._bufs.get(k.key[0])
            k.graph.replay()
            self.stats["replays"] += 1
        k.total_host.copy_(k.det["crop_total"], non_blocking=True)
        self.stream.synchronize()
        return int(k.total_host[0])

    def _classify_graph(self, k: _Key, capacity: int) -> _Stage2:
        s = k.stage2.get(capacity)
        if s is None:
            s = _Stage2()
            s.graph, (s.out, s.packed) = self._captured(lambda: self._stage2(k, capacity))
            s.host = torch.zeros(tuple(s.packed.shape), dtype=torch.int32).pin_memory()
            s.bufs = [v._bufs.get((capacity, 0)) for v in self.vits]
            k.stage2[capacity] = s
        return s

    def _classify(self, k: _Key, capacity: int) -> np.ndarray:
        with self._vit_guards():
            s = self._classify_graph(k, capacity)
            s.graph.replay()
            self.stats["replays"] += 1
        s.host.copy_(s.packed, non_blocking=True)
        self.stream.synchronize()
        return s.host.numpy()

    # ---------------------------------------------------------------------------------------------------- calls
    def run(self, arrs, timing: Optional[dict] = None) -> Dict[str, np.ndarray]:
        """timing: a dict that receives the host seconds of "stage1" (uploads to the crop count) and "stage2" (to the records)."""
        import time
        from .pipeline import fit_capacity
        arrs = check_images(arrs)
        with self._lock, torch.cuda.stream(self.stream):
            t0 = time.perf_counter()
            self._refreeze()
            B = len(arrs)
            k = self._key(session_key(B, max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs)))
            canvas = k.canvas_host.numpy()
            for i, a in enumerate(arrs):
                canvas[i, :a.shape[0], :a.shape[1]] = a
            request_block([a.shape[:2] for a in arrs], self._net()[0], out=k.block_host.numpy())
            k.canvas.copy_(k.canvas_host, non_blocking=True)
            k.block.copy_(k.block_host, non_blocking=True)
            total = self._detect(k)
            t1 = time.perf_counter()
            capacity = fit_capacity(total, k.det["capacity"])
            self.last = {"key": k.key, "capacity": capacity, "total": total}
            if capacity == 0:
                res = empty_results(self.nc)
            else:
                res = unpack_results(self._classify(k, capacity), self.nc)
            if timing is not None:
                timing["stage1"], timing["stage2"] = t1 - t0, time.perf_counter() - t1
            return res

    def warm(self, B: int, hw: Tuple[int, int], capacities: Optional[Sequence[int]] = None):
        """Captures the stage-1 key of B images of at most hw = (h, w) and its stage-2 keys for `capacities` (None: every
        capacity fit_capacity can give for this B), on whatever the canvas holds."""
        from .pipeline import fit_capacity
        h, w = hw
        with self._lock, torch.cuda.stream(self.stream):
            self._refreeze()
            k = self._key(session_key(B, h, w))
            request_block([(h, w)] * B, self._net()[0], out=k.block_host.numpy())
            k.block.copy_(k.block_host, non_blocking=True)
            self._detect(k)
            cap = k.det["capacity"]
            if capacities is None:
                capacities = sorted({fit_capacity(t, cap) for t in range(1, cap + 1)})
            for c in capacities:
                if c != fit_capacity(c, cap) or c <= 0:
                    raise YvError(f"warm: {c} is no capacity fit_capacity gives for at most {cap} crops")
                with self._vit_guards():
                    self._classify_graph(k, c)
            self.stream.synchronize()

    def matches(self, pipe) -> bool:
        """True where the session's engines ARE pipe's objects (a retrained module builds new engines) and pipe would freeze what
        the session's pipeline freezes."""
        return (self.yolo is pipe.yolo and len(self.vits) == len(pipe.vits) and all(a is b for a, b in zip(self.vits, pipe.vits))
                and frozen_state(pipe) == frozen_state(self.pipe))
