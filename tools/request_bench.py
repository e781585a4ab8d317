#!/usr/bin/env python3
"""Dev tool (GPU box): latency of ONE DetectClassifyPipeline.__call__ at request size - what inferdet.main runs per chunk - for
YOLOv8n + ViT-B/16 and YOLOv8n + ViT-B/8 at B = 1 and 4 images of 640 x 640 with 1, 3 and 8 detections per image, in ten states:
  default              the pipeline as it ships (classifier capacity B * topk = 100 B crops);
  fit_crops            DetectClassifyPipeline(fit_crops=True);
  fit_crops+mid_gemm   ... with VitEngine(mid_gemm=True);
  mid_gemm             VitEngine(mid_gemm=True) alone;
  small_maps           YoloEngine(small_maps=True) alone (a sibling of the detector: the same weights);
  fit+mid+small_maps   ... on top of fit_crops + mid_gemm;
  grouped_head         YoloEngine(grouped_head=True) alone (likewise a sibling);
  fit+mid+small_maps+grouped   every switch of the above;
  fit+mid+ln_gemm      VitEngine(mid_gemm=True, ln_gemm=True) on top of fit_crops;
  fit+mid+small+grouped+ln     ... and on top of every switch.
RB_MODELS (comma-separated classifier names) restricts the classifiers, RB_STATES (comma-separated labels) the states; the ratio
column is against "default" where that state runs, else against the first state, and an ln_gemm state is also set against the
same state without the flag.
The detector runs on the images (its time is part of the call); the NMS then works on a synthetic candidate set in place of the
random-weight detector's - 8400 boxes per image by the recipe of bench.py's postproc mode (centres uniform, sides U[16, 256]),
with exactly d well-separated candidates above the thresholds - so that the crop count is the one asked for.
The states are interleaved in one process, RB_RUNS (3) runs of RB_CALLS (20) calls each; a call is timed on the host from its
start to the end of a device synchronisation.  Reported: the median call; the median detect stage alone (same method, once for
each detector - unflagged, small_maps, grouped_head, both - and each state is listed with its own detector's); the launches of one
detect stage, DERIVED, not observed: the entries of the detector's launch list, a ConvGroup entry counted as the launches that
yvhip.conv2d_group_plan - the partition function of the launch itself - reports for it under the pass's options, plus the tail's
one; and the peak of torch.cuda.max_memory_allocated over a call above what was allocated before the first call of that shape
(the engines' activation buffers: every engine starts each shape with none).
--e2e times instead host arrays in to records out - inferdet.run_chunk, eager, against yvhip.request.RequestSession.run, two graph
replays - at the same shapes (end_to_end; RB_ROWS restricts its rows); profiles/request_bench_graph.txt is its output.
--e2e --mx: the rows of an mxfp8 classifier - VitEngine(dtype="mxfp8") without and with mid_gemm, eager and in a session - beside the
bf16 rows with mid_gemm, in the same process; each mxfp8 row is also set against its twin (the same row without mid_gemm; for the
rows without it, the bf16 row of the same kind); profiles/request_bench_mx.txt is its output."""
import gc, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip
from yvhip import engines
from yvhip.pipeline import DetectClassifyPipeline

dev = "cuda:0"
RUNS = int(os.environ.get("RB_RUNS", 3))
CALLS = int(os.environ.get("RB_CALLS", 20))
S, A, NC = 640, 8400, 5
# (label, fit_crops, (mid_gemm, ln_gemm), (small_maps, grouped_head))
STATES = [("default", False, (False, False), (False, False)), ("fit_crops", True, (False, False), (False, False)),
          ("fit_crops+mid_gemm", True, (True, False), (False, False)), ("mid_gemm", False, (True, False), (False, False)),
          ("small_maps", False, (False, False), (True, False)), ("fit+mid+small_maps", True, (True, False), (True, False)),
          ("grouped_head", False, (False, False), (False, True)), ("fit+mid+small_maps+grouped", True, (True, False), (True, True)),
          ("fit+mid+ln_gemm", True, (True, True), (False, False)), ("fit+mid+small+grouped+ln", True, (True, True), (True, True))]
WITHOUT_LN = {"fit+mid+ln_gemm": "fit_crops+mid_gemm", "fit+mid+small+grouped+ln": "fit+mid+small_maps+grouped"}
if os.environ.get("RB_STATES"):
    STATES = [s for s in STATES if s[0] in os.environ["RB_STATES"].split(",")]
DETECTORS = [w for w in [(False, False), (True, False), (False, True), (True, True)] if any(s[3] == w for s in STATES)]
MODELS = [m for m in os.environ.get("RB_MODELS", "vit_base_patch16_224,vit_base_patch8_224").split(",") if m]


def candidates(B, d, seed=4321):
    """(boxes (B, A, 4), scores (B, A, NC)): d disjoint 96 x 96 boxes per image score 0.9, every other candidate 0.01."""
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand(B, A, 2, generator=g) * S
    wh = torch.rand(B, A, 2, generator=g) * 240 + 16
    boxes = torch.cat([(ctr - wh / 2).clamp(0, S), (ctr + wh / 2).clamp(0, S)], -1).contiguous()
    scores = torch.full((B, A, NC), 0.01)
    for b in range(B):
        for k in range(d):
            x0, y0 = 16 + (k % 4) * 150, 16 + (k // 4) * 150
            boxes[b, k] = torch.tensor([x0, y0, x0 + 96, y0 + 96], dtype=torch.float32)
            scores[b, k, (b + k) % NC] = 0.9
    return boxes.to(dev), scores.to(dev)


def with_candidates(pipe, boxes, scores):
    """pipe.detect: the detector runs (and is timed), the NMS sees the synthetic candidates."""
    def detect(images):
        pipe.yolo(images)
        return yvhip.efficient_nms(boxes, scores, pipe.score_threshold, pipe.iou_threshold, pipe.topk)
    pipe.detect = detect


def wall(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def detect_launch_count(eng, B):
    """Launches of one detect stage of `eng` at B images: see the module text."""
    H, W = eng.hw
    tail = not eng.fused_tail
    old = yvhip.get_option("conv_small")
    if eng.small_maps:
        yvhip.set_option("conv_small", engines.SMALL_MAP_PIXELS)
    try:
        n = 1                                                  # detect_tail / detect_decode
        for e in engines.detect_launches(eng.scale, eng.nc, True, tail, eng.grouped_head):
            if type(e) is engines.ConvGroup:
                bufs = eng._buffers(B)["flat"]
                n += yvhip.conv2d_group_plan([(B, H // c.down, W // c.down, c.k, c.stride, c.srcs[0][2], 0, c.cout,
                                               bufs[c.out].shape[-1], 0, c.flags) for c in e.convs])[0]
            else:
                n += 1
    finally:
        yvhip.set_option("conv_small", old)
    return n


def trace_one():
    """--trace: two default-state calls (B = 1, 3 detections, ViT-B/16) and nothing else, for a kernel trace of the default path
    (rocprofv3 --kernel-trace -- python tools/request_bench.py --trace); uses nothing that an earlier commit lacks."""
    yolo = engines.YoloEngine(engines.init_yolo_state("n", NC, seed=42, head_gain=4.0), "n", NC, S, device=dev)
    name = "vit_base_patch16_224"
    vit = engines.VitEngine(engines.init_vit_wrapper_state(name, NC, seed=42), name, NC, device=dev)
    pipe = DetectClassifyPipeline(yolo, [vit])
    with_candidates(pipe, *candidates(1, 3))
    images = torch.randint(0, 256, (1, S, S, 3), generator=torch.Generator().manual_seed(1234), dtype=torch.uint8).to(dev)
    for _ in range(2):
        out = pipe(images)
    torch.cuda.synchronize()
    print("crops", int(out["crop_total"][0]), "labels", out["cls_label"][:3].tolist())


def main():
    print(f"# {torch.cuda.get_device_name(0)}; ms per call, median of {RUNS} x {CALLS} calls, states interleaved; "
          f"memory: peak above the allocation before the shape's first call")
    print(f"# {'classifier':22s} {'B':>2s} {'dets':>4s} {'crops':>5s}  {'state':20s} {'capacity':>8s} {'call ms':>8s} {'detect ms':>9s} "
          f"{'classify ms':>11s} {'peak MB':>9s}  call / default  detect launches (derived from the launch list and conv2d_group_plan, not observed)")
    yolo_sd = engines.init_yolo_state("n", NC, seed=42, head_gain=4.0)
    yolo = engines.YoloEngine(yolo_sd, "n", NC, S, device=dev, small_maps=False)
    dets = {}
    for small, grouped in [(False, False)] + [w for w in DETECTORS if any(w)]:
        dets[(small, grouped)] = e = yolo if not (small or grouped) else yolo.resized(S)
        e.small_maps, e.grouped_head = small, grouped
    g = torch.Generator().manual_seed(1234)
    for name in MODELS:
        vit_sd = engines.init_vit_wrapper_state(name, NC, seed=42)
        vits = {k: engines.VitEngine(vit_sd, name, NC, device=dev, mid_gemm=k[0], ln_gemm=k[1]) for k in sorted({s[2] for s in STATES})}
        for B in (1, 4):
            images = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
            for d in (1, 3, 8):
                boxes, scores = candidates(B, d)
                for e in dets.values():                       # the detectors' own buffers for this B exist before anything is measured
                    e(images)
                pipes, peak, cap, crops = {}, {}, {}, {}
                for label, fit, mid, which in STATES:
                    pipes[label] = p = DetectClassifyPipeline(dets[which], [vits[mid]], fit_crops=fit)
                    with_candidates(p, boxes, scores)
                for label, fit, mid, which in STATES:         # memory: each state from engines without activation buffers
                    for v in vits.values():
                        v._bufs.clear()
                    gc.collect(); torch.cuda.synchronize(); torch.cuda.empty_cache()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    out = pipes[label](images)
                    torch.cuda.synchronize()
                    peak[label] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    cap[label], crops[label] = out["capacity"], int(out["crop_total"][0])
                    if crops[label] != B * d:
                        print(f"# note: {label}: {crops[label]} crops where {B * d} were injected")
                    del out
                for label, *_ in STATES:                      # buffers of every state back in place, then warm
                    wall(lambda: pipes[label](images), 3)
                call = {label: [] for label, *_ in STATES}
                det = {which: [] for which in DETECTORS}
                first = {which: next(label for label, _, _, w in STATES if w == which) for which in DETECTORS}
                for rd in range(RUNS):
                    for label, *_ in STATES:
                        call[label] += wall(lambda: pipes[label](images), CALLS)
                    for which in DETECTORS:
                        det[which] += wall(lambda: pipes[first[which]].detect_stage(images), CALLS)
                t0 = median(call["default" if "default" in call else STATES[0][0]])
                for label, _, _, which in STATES:
                    t, t_det = median(call[label]), median(det[which])
                    twin = WITHOUT_LN.get(label)
                    vs = f"  x {t / median(call[twin]):.3f} of {twin}" if twin in call else ""
                    print(f"  {name:22s} {B:2d} {d:4d} {crops[label]:5d}  {label:20s} {cap[label]:8d} {t:8.3f} {t_det:9.3f} "
                          f"{t - t_det:11.3f} {peak[label]:9.1f}  {t / t0:6.2f}  {detect_launch_count(dets[which], B):15d}{vs}", flush=True)
                del pipes


# --e2e rows: (label, session?, fit_crops, mid_gemm, (small_maps, grouped_head))
E2E_ROWS = [("eager chunk", False, False, False, (False, False)),
            ("eager chunk fit+mid", False, True, True, (False, False)),
            ("eager chunk fit+mid+small+grouped", False, True, True, (True, True)),
            ("session", True, True, False, (False, False)),
            ("session mid", True, True, True, (False, False)),
            ("session small+grouped", True, True, False, (True, True)),
            ("session mid+small+grouped", True, True, True, (True, True))]
# --e2e --mx rows: the same fields and the classifier's dtype; E2E_TWIN: the row each is also set against
E2E_MX_ROWS = [("eager fit+mid bf16", False, True, True, (False, False), "bf16"),
               ("session mid bf16", True, True, True, (False, False), "bf16"),
               ("eager fit mxfp8", False, True, False, (False, False), "mxfp8"),
               ("eager fit+mid mxfp8", False, True, True, (False, False), "mxfp8"),
               ("session mxfp8", True, True, False, (False, False), "mxfp8"),
               ("session mid mxfp8", True, True, True, (False, False), "mxfp8")]
E2E_TWIN = {"eager fit mxfp8": "eager fit+mid bf16", "eager fit+mid mxfp8": "eager fit mxfp8", "session mxfp8": "session mid bf16",
            "session mid mxfp8": "session mxfp8"}
E2E_CAND = {}                                                       # B -> (boxes, scores): static, the scores rewritten in place


def e2e_candidates(B, d):
    """candidates(B, 8)'s boxes once per B; the scores of the first d per image raised in place (a captured graph reads them)."""
    if B not in E2E_CAND:
        boxes, _ = candidates(B, 8)
        E2E_CAND[B] = (boxes, torch.full((B, A, NC), 0.01, device=dev))
    s = torch.full((B, A, NC), 0.01)
    for b in range(B):
        for k in range(d):
            s[b, k, (b + k) % NC] = 0.9
    E2E_CAND[B][1].copy_(s)
    torch.cuda.synchronize()


def e2e_detect(pipe):
    def detect(images):
        pipe.yolo(images)
        boxes, scores = E2E_CAND[images.shape[0]]
        return yvhip.efficient_nms(boxes, scores, pipe.score_threshold, pipe.iou_threshold, pipe.topk)
    pipe.detect = detect
    return pipe


def end_to_end():
    """--e2e: host arrays in to records out, per chunk of B images of 640 x 640 - what inferdet.main does per chunk besides reading
    the files: the eager chunk function (inferdet.run_chunk: canvas + four geometry uploads, letterbox, the pipeline call, seven
    reads) against yvhip.request.RequestSession.run (one canvas + one block upload, two graph replays, one count read, one record
    download) over the same engines, rows interleaved in one process, same shapes and method as the ten states.  A session is
    built once per row and classifier and keeps its keys across B and detections, as a server's would.  Reported: the median
    call; the session's two stages apart (host clock: uploads -> crop count, -> records); per key's first visit (eager warm-up,
    capture, first replay) the peak of torch.cuda.max_memory_allocated above the allocation before it, what stays allocated after
    it, and the growth of the reserved pool - the engines' buffer sets of that size exist before (an eager fitted chunk on the same
    engines runs first), the session's stream has its workspace, so this is the static buffers and the graphs' pools."""
    from YOLOTensorRT.inferdet import run_chunk
    from yvhip.request import RequestSession
    rows = [r for r in (E2E_MX_ROWS if "--mx" in sys.argv[1:] else E2E_ROWS)
            if not os.environ.get("RB_ROWS") or r[0] in os.environ["RB_ROWS"].split(",")]
    rows = [tuple(r) + ("bf16",) * (6 - len(r)) for r in rows]
    print(f"# {torch.cuda.get_device_name(0)}; host arrays in -> records out, ms per chunk, median of {RUNS} x {CALLS} calls, rows "
          f"interleaved; memory in MB at the first visit of the row's key (B, 640, 640, capacity)")
    print(f"# {'classifier':22s} {'B':>2s} {'dets':>4s} {'crops':>5s}  {'row':34s} {'capacity':>8s} {'call ms':>8s} {'stage1 ms':>9s} "
          f"{'stage2 ms':>9s}  {'/ eager':>7s} {'/ fit+mid':>9s}  {'peak MB':>8s} {'held MB':>8s} {'reserved MB':>11s}")
    yolo = engines.YoloEngine(engines.init_yolo_state("n", NC, seed=42, head_gain=4.0), "n", NC, S, device=dev, small_maps=False)
    dets = {(False, False): yolo}
    if any(r[4] == (True, True) for r in rows):
        dets[(True, True)] = e = yolo.resized(S)
        e.small_maps, e.grouped_head = True, True
    g = torch.Generator().manual_seed(1234)
    for name in MODELS:
        vit_sd = engines.init_vit_wrapper_state(name, NC, seed=42)
        vits = {k: engines.VitEngine(vit_sd, name, NC, device=dev, mid_gemm=k[0], dtype=k[1]) for k in sorted({(r[3], r[5]) for r in rows})}
        pipes, sessions, fitted = {}, {}, {}
        for label, ses, fit, mid, which, dtype in rows:
            pipes[label] = e2e_detect(DetectClassifyPipeline(dets[which], [vits[(mid, dtype)]], fit_crops=fit))
            if ses:
                fitted[label] = e2e_detect(DetectClassifyPipeline(dets[which], [vits[(mid, dtype)]], fit_crops=True))
                sessions[label] = s = RequestSession(pipes[label])
                with torch.cuda.stream(s.stream):
                    yvhip._st()                                   # the stream's split-K workspace: not a cost of a key
        seen = set()
        for B in (1, 4):
            arrs = [a.numpy() for a in torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)]
            for d in (1, 3, 8):
                e2e_candidates(B, d)
                timing = {label: [] for label in sessions}

                def call(label):
                    if label in sessions:
                        t = {}
                        rec = sessions[label].run(arrs, timing=t)
                        timing[label].append(t)
                        return len(rec["image"])
                    return len(run_chunk(pipes[label], arrs, (S, S), S, dev)[4])
                mem, crops, cap = {}, {}, {}
                for label, ses, *_ in rows:                     # first visits
                    if ses:                                     # the engines' buffer sets of this size exist before the key is made
                        run_chunk(fitted[label], arrs, (S, S), S, dev)
                    gc.collect(); torch.cuda.synchronize(); torch.cuda.empty_cache()
                    base, rbase = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
                    torch.cuda.reset_peak_memory_stats()
                    crops[label] = call(label)
                    torch.cuda.synchronize()
                    key = (label, B, sessions[label].last["capacity"]) if ses else None
                    if ses and key not in seen:
                        seen.add(key)
                        mem[label] = ((torch.cuda.max_memory_allocated() - base) / 2 ** 20, (torch.cuda.memory_allocated() - base) / 2 ** 20,
                                      (torch.cuda.memory_reserved() - rbase) / 2 ** 20)
                    cap[label] = sessions[label].last["capacity"] if ses else "-"
                    if crops[label] != B * d:
                        print(f"# note: {label}: {crops[label]} crops where {B * d} were injected")
                for label, *_ in rows:
                    wall(lambda: call(label), 3)
                for t in timing.values():
                    t.clear()
                ms = {label: [] for label, *_ in rows}
                for rd in range(RUNS):
                    for label, *_ in rows:
                        ms[label] += wall(lambda: call(label), CALLS)
                t0 = median(ms[rows[0][0]])
                t1 = median(ms["eager chunk fit+mid"]) if "eager chunk fit+mid" in ms else None
                for label, ses, *_ in rows:
                    t = median(ms[label])
                    st = (f"{median([x['stage1'] for x in timing[label]]) * 1e3:9.3f} {median([x['stage2'] for x in timing[label]]) * 1e3:9.3f}"
                          if ses else f"{'-':>9s} {'-':>9s}")
                    m = "  ".join(f"{v:8.1f}" for v in mem[label]) if label in mem else ""
                    r1 = f"{t / t1:9.2f}" if t1 else f"{'-':>9s}"
                    twin = E2E_TWIN.get(label)
                    vs = f"  x {t / median(ms[twin]):.3f} of {twin}" if twin in ms else ""
                    print(f"  {name:22s} {B:2d} {d:4d} {crops[label]:5d}  {label:34s} {str(cap[label]):>8s} {t:8.3f} {st}  {t / t0:7.2f} {r1}  {m}{vs}",
                          flush=True)
        for label, s in sessions.items():
            print(f"# {name}, {label}: stats {s.stats}, keys {[(k, sorted(v.stage2)) for k, v in s.keys.items()]}")
        del pipes, sessions, fitted


if __name__ == "__main__":
    args = sys.argv[1:]
    trace_one() if "--trace" in args else end_to_end() if "--e2e" in args else main()
