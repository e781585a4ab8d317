"""GPU: yv_pack_results and yvhip.request.RequestSession / inferdet.main(graph=True).  Every comparison
is exact: a replay launches the kernels of the eager stages on the same data.  The reference of a session call is
tests/request_reference.pack_ref of what the eager DetectClassifyPipeline(fit_crops=True) gives on the same images."""
import os

import numpy as np
import pytest
import torch

import request_reference as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME, NC, S, B, R = "vit_tiny_test", 5, 128, 2, 3
A = 64                                         # synthetic candidates per image
FIELDS = ("image", "slot", "box", "det_label", "cls_label", "score", "logits")


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module")
def engines_(yv):
    from yvhip import engines
    yolo = engines.YoloEngine(engines.init_yolo_state("n", NC, seed=1, head_gain=4.0), "n", NC, S, DEV)
    vit = engines.VitEngine(engines.init_vit_wrapper_state(NAME, NC, seed=2), NAME, NC, device=DEV)
    return yolo, vit


# ---------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("shape", [(3, 5, 8, 5), (1, 1, 1, 1), (2, 4, 6, 7)])
def test_pack_results_against_the_reference(yv, shape):
    from yvhip import request
    Bn, slots, cap, nc = shape
    g = np.random.default_rng(sum(shape))
    crop_list = np.zeros((cap, 6), dtype=np.int32)
    crop_list[:, 0], crop_list[:, 5] = np.sort(g.integers(0, Bn, cap)), g.integers(0, slots, cap)
    crop_list[:, 1:5] = g.integers(0, 500, (cap, 4))
    det = dict(det_box=g.integers(-5, 2000, (Bn, slots, 4)).astype(np.int32),
               det_score=g.random((Bn, slots), dtype=np.float32),
               det_label=g.integers(0, 80, (Bn, slots)).astype(np.int32))
    cls_logits = g.standard_normal((cap, nc)).astype(np.float32)
    cls_label = g.integers(0, nc, cap).astype(np.int32)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in det.items()}
    dev["crop_list"] = torch.from_numpy(crop_list).to(DEV)
    lab, lg = torch.from_numpy(cls_label).to(DEV), torch.from_numpy(cls_logits).to(DEV)
    for total in sorted({0, 1, cap - 1, cap}):
        dev["crop_total"] = torch.tensor([total], dtype=torch.int32, device=DEV)
        want = rr.pack_ref(crop_list, [total], det["det_box"], det["det_score"], det["det_label"], cls_label, cls_logits, cap)
        out = torch.full((1 + cap, 9 + nc), 0x5A5A5A5A, dtype=torch.int32, device=DEV)      # rows past total must be zeroed
        got = yv.pack_results(dev, lab, lg, cap, out=out)
        assert got is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), (shape, total)
        assert np.array_equal(yv.pack_results(dev, lab, lg, cap).cpu().numpy(), want)
        rec = request.unpack_results(want, nc)
        assert len(rec["image"]) == total and np.array_equal(rec["logits"], cls_logits[:total])
    dev["crop_total"] = torch.tensor([cap + 3], dtype=torch.int32, device=DEV)              # a count past cap: the first cap rows
    assert int(yv.pack_results(dev, lab, lg, cap)[0, 0]) == cap
    head = yv.pack_results(dev, lab, lg, 0).cpu().numpy()                                   # cap == 0: the header only
    assert head.tolist() == [[0, Bn, slots, 0, nc] + [0] * (4 + nc)]
    with pytest.raises(yv.YvError):
        yv.pack_results(dev, lab, lg, cap + 1)
    with pytest.raises(yv.YvError):
        yv.pack_results(dev, lab, lg, cap, out=torch.zeros((cap, 9 + nc), dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------- 2. sessions
class _Candidates:
    """Synthetic NMS input for pipelines at S = 128, as tools/request_bench.py feeds it: three disjoint boxes per image, of which
    the first counts[b] of image b score above the thresholds after set()."""
    BOXES = ((20, 20, 45, 50), (50, 20, 75, 50), (80, 60, 105, 95))

    def __init__(self, yv):
        g = torch.Generator().manual_seed(11)
        ctr, wh = torch.rand(B, A, 2, generator=g) * S, torch.rand(B, A, 2, generator=g) * 40 + 8
        boxes = torch.cat([(ctr - wh / 2).clamp(0, S), (ctr + wh / 2).clamp(0, S)], -1)
        for b in range(B):
            boxes[b, :R] = torch.tensor(self.BOXES, dtype=torch.float32)
        self.yv, self.boxes = yv, boxes.contiguous().to(DEV)
        self.scores = torch.full((B, A, NC), 0.01, device=DEV)

    def set(self, counts):
        s = torch.full((B, A, NC), 0.01)
        for b, d in enumerate(counts):
            for k in range(d):
                s[b, k, (b + k) % NC] = 0.9 - 0.1 * k
        self.scores.copy_(s)                                  # in place: a captured graph reads this tensor

    def attach(self, pipe):
        def detect(images):
            pipe.yolo(images)
            return self.yv.efficient_nms(self.boxes, self.scores, pipe.score_threshold, pipe.iou_threshold, pipe.topk)
        pipe.detect = detect
        return pipe


def _eager(yv, pipe, arrs):
    """inferdet.main's chunk on the eager pipeline (tight canvas, four geometry tensors): the outputs on the host."""
    from YOLOTensorRT.models.utils import letterbox_geometry
    Hc, Wc = max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs)
    canvas = np.zeros((len(arrs), Hc, Wc, 3), dtype=np.uint8)
    geom, ratio, dwdh, wh = [], [], [], []
    Hn, Wn = pipe.yolo.hw
    for i, a in enumerate(arrs):
        h, w = a.shape[:2]
        canvas[i, :h, :w] = a
        r, (dw, dh), (nw, nh), (left, top) = letterbox_geometry(h, w, (Wn, Hn))
        geom.append([w, h, nw, nh, left, top]); ratio.append(r); dwdh += [dw, dh]; wh += [w, h]
    src = torch.from_numpy(canvas).to(DEV)
    net_in = yv.letterbox(src, torch.tensor(geom, dtype=torch.int32, device=DEV), pipe.yolo.size)
    out = pipe(net_in, torch.tensor(ratio, dtype=torch.float32, device=DEV), torch.tensor(dwdh, dtype=torch.float32, device=DEV),
               torch.tensor(wh, dtype=torch.int32, device=DEV), src_images=src)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _want(out):
    from yvhip import request
    words = rr.pack_ref(out["crop_list"], out["crop_total"], out["det_box"], out["det_score"], out["det_label"], out["cls_label"],
                        out["cls_logits"], out["capacity"])
    return request.unpack_results(words, NC)


def _same(got, want):
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
        assert got[f].tobytes() == want[f].tobytes(), f


def _pictures(g, sizes):
    return [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


@pytest.fixture()
def pipes(yv, engines_):
    """(candidates, the session's pipeline, the eager fit_crops pipeline) on the same engines and the same candidates."""
    from yvhip.pipeline import DetectClassifyPipeline
    yolo, vit = engines_
    cand = _Candidates(yv)
    return (cand, cand.attach(DetectClassifyPipeline(yolo, [vit], max_crops_per_image=R)),
            cand.attach(DetectClassifyPipeline(yolo, [vit], max_crops_per_image=R, fit_crops=True)))


def test_session_against_the_eager_pipeline(yv, pipes):
    from yvhip.request import RequestSession
    cand, pipe, eager = pipes
    ses = RequestSession(pipe)
    g = np.random.default_rng(21)
    sizes = [(120, 128), (128, 100)]
    caps = []
    for d in (3, 0, 1, 3, 2, 0, 3):
        cand.set((d, d))
        arrs = _pictures(g, sizes)                            # new source pixels in every call
        want = _eager(yv, eager, arrs)
        assert int(want["crop_total"][0]) == 2 * d            # the candidates give the crops asked for
        got = ses.run(arrs)
        _same(got, _want(want))
        assert len(got["image"]) == 2 * d and ses.last["capacity"] == want["capacity"]
        caps.append(want["capacity"])
    assert caps == [6, 0, 2, 6, 4, 0, 6]
    # distinct keys visited: one stage-1 key and the capacities 6, 2, 4; replays: seven detect stages and five classifier stages
    assert ses.stats == {"eager": 4, "captures": 4, "replays": 12, "evictions": 0}
    assert list(ses.keys) == [(B, 128, 128)] and sorted(ses.keys[(B, 128, 128)].stage2) == [2, 4, 6]
    # fewer crops on a graph that has shown more: 6 crops, then 5 and 1 + 3 on the same capacity-6 / capacity-4 graphs
    for counts, cap in (((3, 3), 6), ((3, 2), 6), ((2, 2), 4), ((1, 2), 4), ((1, 0), 1)):
        cand.set(counts)
        arrs = _pictures(g, sizes)
        got = ses.run(arrs)
        _same(got, _want(_eager(yv, eager, arrs)))
        total = sum(counts)
        words = ses.keys[(B, 128, 128)].stage2[cap].host.numpy()
        assert words.shape == (1 + cap, 9 + NC) and words[0, 0] == total and not words[1 + total:].any()
    assert ses.stats["captures"] == 5 and ses.stats["replays"] == 22
    with pytest.raises(yv.YvError):
        ses.run([])
    with pytest.raises(yv.YvError):
        ses.run([np.zeros((8, 8, 3), dtype=np.float32)])


def test_results_belong_to_the_caller(yv, pipes):
    """The records of a one-crop request - one row, the shape numpy hands out as a view - do not change when the next request
    downloads into the session's pinned buffer."""
    from yvhip.request import RequestSession
    cand, pipe, eager = pipes
    ses = RequestSession(pipe)
    cand.set((1, 0))
    g = np.random.default_rng(26)
    sizes = [(128, 128), (128, 128)]
    first_arrs, second_arrs = _pictures(g, sizes), _pictures(g, sizes)
    first = ses.run(first_arrs)
    assert len(first["image"]) == 1 and ses.last["capacity"] == 1
    held = {f: first[f].copy() for f in FIELDS}
    host = ses.keys[(B, 128, 128)].stage2[1].host.numpy()
    assert not any(np.shares_memory(first[f], host) for f in FIELDS)
    second = ses.run(second_arrs)
    _same(first, held)
    _same(first, _want(_eager(yv, eager, first_arrs)))
    _same(second, _want(_eager(yv, eager, second_arrs)))
    assert first["logits"].tobytes() != second["logits"].tobytes()             # other pixels: the buffer did change


def test_flipped_attribute_captures_again(yv, pipes):
    """What a capture froze (frozen_state) is compared at every run: conf raised between two calls drops the keys."""
    from yvhip.request import RequestSession
    cand, pipe, eager = pipes
    ses = RequestSession(pipe)
    cand.set((3, 3))                                                           # scores 0.9, 0.8, 0.7 per image
    g = np.random.default_rng(27)
    arrs = _pictures(g, [(128, 128), (128, 128)])
    _same(ses.run(arrs), _want(_eager(yv, eager, arrs)))
    assert ses.stats == {"eager": 2, "captures": 2, "replays": 2, "evictions": 0} and ses.last["total"] == 6
    pipe.conf = eager.conf = 0.85
    got = ses.run(arrs)
    _same(got, _want(_eager(yv, eager, arrs)))
    assert len(got["image"]) == 2 and ses.stats == {"eager": 4, "captures": 4, "replays": 4, "evictions": 1}
    pipe.vits[0].cls_tail = False                                              # an engine attribute its launch list reads
    try:
        _same(ses.run(arrs), _want(_eager(yv, eager, arrs)))
        assert ses.stats["evictions"] == 2 and ses.stats["captures"] == 6
    finally:
        pipe.vits[0].cls_tail = True


def test_stale_canvas_is_never_read(yv, pipes):
    from yvhip.request import RequestSession
    cand, pipe, eager = pipes
    ses = RequestSession(pipe)
    cand.set((3, 2))
    arrs = _pictures(np.random.default_rng(22), [(128, 90), (100, 128)])      # both smaller than the (2, 128, 128) canvas
    first = ses.run(arrs)
    k = ses.keys[(B, 128, 128)]
    for buf in (k.canvas_host, k.canvas):
        for i, a in enumerate(arrs):
            buf[i, a.shape[0]:, :] = 255
            buf[i, :, a.shape[1]:] = 255
    torch.cuda.synchronize()
    second = ses.run(arrs)
    _same(second, first)
    _same(second, _want(_eager(yv, eager, arrs)))
    assert len(second["image"]) == 5
    host = k.canvas_host.numpy()
    assert (host[0, :, 90:] == 255).all() and (host[1, 100:] == 255).all()    # the session cleared nothing


def test_sizes_share_keys_and_eviction_recaptures(yv, pipes):
    from yvhip.request import RequestSession
    cand, pipe, eager = pipes
    ses = RequestSession(pipe, max_keys=1)
    g = np.random.default_rng(23)
    cand.set((0, 0))                                                           # no crops: the detect stage's graph alone
    for sizes in ([(120, 128), (128, 100)], [(65, 128), (100, 70)], [(128, 65), (1, 1)]):      # three sizes, one rounded key
        arrs = _pictures(g, sizes)
        got = ses.run(arrs)
        _same(got, _want(_eager(yv, eager, arrs)))
        assert len(got["image"]) == 0
    assert ses.stats == {"eager": 1, "captures": 1, "replays": 3, "evictions": 0} and list(ses.keys) == [(B, 128, 128)]
    cand.set((1, 1))
    first_arrs = _pictures(g, [(120, 128), (128, 100)])
    first = ses.run(first_arrs)
    _same(first, _want(_eager(yv, eager, first_arrs)))
    assert len(first["image"]) == 2 and ses.stats["captures"] == 2             # + capacity 2
    small = _pictures(g, [(64, 60), (50, 64)])                                 # another key: captured, the first one evicted
    want_small = _eager(yv, eager, small)
    _same(ses.run(small), _want(want_small))
    assert ses.stats["evictions"] == 1 and list(ses.keys) == [(B, 64, 64)]
    n = ses.stats["captures"]
    assert n == 3 + (want_small["capacity"] > 0)                               # stage 1, and the classifier stage of its crops
    again = ses.run(first_arrs)                                                # back: captured again, the same records
    _same(again, first)
    assert ses.stats["captures"] == n + 2 and ses.stats["evictions"] == 2 and list(ses.keys) == [(B, 128, 128)]
    ses.warm(B, (128, 128), capacities=[1, 6])
    assert sorted(ses.keys[(B, 128, 128)].stage2) == [1, 2, 6] and ses.stats["captures"] == n + 4
    _same(ses.run(first_arrs), first)
    with pytest.raises(yv.YvError):
        ses.warm(B, (128, 128), capacities=[5])


def test_threads_share_a_session(yv, pipes):
    """Request threads call without a lock of their own (the reference's Flask handlers): run() serialises them, also through
    the first visit of a key, and each gets the records of its own images."""
    import threading
    from yvhip.request import RequestSession
    cand, pipe, eager = pipes
    cand.set((2, 1))
    g = np.random.default_rng(25)
    jobs = [_pictures(g, [(128, 128), (100, 128)]) for _ in range(6)]
    want = [_want(_eager(yv, eager, arrs)) for arrs in jobs]
    ses = RequestSession(pipe)
    got, errors = [None] * len(jobs), []

    def worker(ids):
        try:
            for i in ids:
                got[i] = ses.run(jobs[i])
        except Exception as e:                                                 # noqa: BLE001 - reported below
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(ids,)) for ids in ((0, 2, 4), (1, 3, 5))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    for a, b in zip(got, want):
        _same(a, b)
    assert ses.stats == {"eager": 2, "captures": 2, "replays": 12, "evictions": 0}


# ---------------------------------------------------------------------------------------------------------- 5. main
class _CFG:
    num_classes, device, modelName, pretrained = NC, DEV, NAME, None


def test_main_graph_against_main(yv, tmp_path):
    import utils.utils as uu
    from PIL import Image
    from test_gpu_rect import _block_image, _cell_detector_state
    from YOLOTensorRT.inferdet import main
    from YOLOTensorRT.models import TRTModule
    from yvhip import engines
    eng = TRTModule(_cell_detector_state(), torch.device(DEV), size=64)
    nets = []
    for seed in (2, 5):
        wpath = str(tmp_path / f"best_{seed}.pth")
        torch.save(engines.init_vit_wrapper_state(NAME, NC, seed=seed), wpath)
        net = uu.build_model(CFG=_CFG, modelName=NAME, pretrained=wpath)
        net.to(DEV); net.eval()
        nets.append(net)
    sets = {"a": [_block_image(100, 48, 30, 70, 12, 34), _block_image(48, 100, 8, 30, 20, 70), _block_image(64, 64, 16, 44, 16, 44)],
            "b": [_block_image(100, 48, 40, 80, 8, 30), _block_image(48, 100, 10, 32, 30, 80), _block_image(64, 64, 12, 40, 20, 48)]}
    for name, pictures in sets.items():
        (tmp_path / name).mkdir()
        for i, im in enumerate(pictures):
            Image.fromarray(im).save(str(tmp_path / name / f"img_{i}.png"))
    call = lambda d, models, **kw: main(Engine=eng, imgs=str(tmp_path / d), device=torch.device(DEV), model_list=models, **kw)
    want = call("a", nets[:1])
    assert all(len(r["objects"]) > 0 for r in want["output"])
    got = call("a", nets[:1], graph=True)
    assert got == want
    assert got == call("a", nets[:1], fit_crops=True)
    cache = eng.__dict__["_request_sessions"]
    one = (False, False, (id(nets[0]),))
    assert list(cache) == [one]
    ses = cache[one]
    assert list(ses.keys) == [(3, 128, 128)]
    seen = set(ses.keys[(3, 128, 128)].stage2)
    assert ses.stats == {"eager": 2, "captures": 2, "replays": 2, "evictions": 0} and len(seen) == 1
    assert call("b", nets[:1], graph=True) == call("b", nets[:1])             # other pictures of the same sizes: a replay
    assert list(cache) == [one] and cache[one] is ses and list(ses.keys) == [(3, 128, 128)]
    new = ses.last["capacity"] not in seen                                     # another crop capacity is another key
    assert ses.last["capacity"] > 0
    assert ses.stats == {"eager": 2 + new, "captures": 2 + new, "replays": 4, "evictions": 0}
    os.environ["YV_REQUEST_GRAPH"] = "1"
    try:
        assert call("a", nets[:1]) == want                                     # the environment variable: the same switch
    finally:
        del os.environ["YV_REQUEST_GRAPH"]
    assert cache[one] is ses and ses.stats["replays"] == 6 and ses.stats["captures"] == 2 + new
    both = call("a", nets)                                                     # an ensemble of two classifiers
    assert call("a", nets, graph=True) == both
    two = (False, False, (id(nets[0]), id(nets[1])))
    assert list(cache) == [one, two] and cache[one] is ses and len(cache[two].vits) == 2      # each list keeps its session
    assert cache[two].stream is ses.stream                                     # one stream (one workspace) per Engine
    assert call("a", nets[:1], graph=True) == want and ses.stats["captures"] == 2 + new       # alternating lists: no re-capture
    eng.score_threshold = 0.3                                                  # a threshold a capture froze: a new session
    try:
        assert call("a", nets[:1], graph=True) == call("a", nets[:1])
        assert cache[one] is not ses
    finally:
        eng.score_threshold = 0.25
    assert call("a", nets[:1], graph=True) == want                             # back at 0.25
    stale = cache[one]
    assert call("a", nets[:1], graph=True) == want and cache[one] is stale
    with torch.no_grad():                                                      # a retrained module builds a new engine
        nets[0].load_state_dict(nets[1].state_dict())
    retrained = call("a", nets[:1])
    assert call("a", nets[:1], graph=True) == retrained
    assert cache[one] is not stale and cache[one].vits[0] is nets[0].engine() and len(cache) == 2
    with pytest.raises(yv.YvError, match="rect"):
        call("a", nets[:1], graph=True, rect=True)


# ---------------------------------------------------------------------------------------------------------- 6. engines after use
def test_eager_use_after_a_session(yv, engines_):
    from yvhip.pipeline import DetectClassifyPipeline
    from yvhip.request import RequestSession
    yolo, vit = engines_
    keys = ("det_count", "det_box", "crop_list", "crop_total", "cls_logits", "cls_label")
    default = DetectClassifyPipeline(yolo, [vit], max_crops_per_image=R)
    img = torch.randint(0, 256, (B, S, S, 3), generator=torch.Generator().manual_seed(31), dtype=torch.uint8).to(DEV)
    opts = ("linear_mid", "conv_small", "linear_ln_mid")
    before_opts = [yv.get_option(o) for o in opts]
    out = default(img)
    torch.cuda.synchronize()
    before = {k: out[k].clone() for k in keys}
    assert int(before["crop_total"][0]) > 0
    ses = RequestSession(DetectClassifyPipeline(yolo, [vit], max_crops_per_image=R))
    g = np.random.default_rng(24)
    for sizes in ([(128, 128), (128, 128)], [(90, 128), (128, 77)]):
        rec = ses.run(_pictures(g, sizes))
    assert ses.stats["replays"] >= 2
    out = default(img)                                                         # the default stream, right after a replay
    rec = ses.run(_pictures(g, [(128, 128), (128, 128)]))                      # and a replay right after an eager step
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(out[k], before[k]), k
    assert [yv.get_option(o) for o in opts] == before_opts
