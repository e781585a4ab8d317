"""GPU: DetectClassifyPipeline(fit_crops=True) / inferdet.main(fit_crops=True) - the classifier sized to the crops of the call
 - against the unfitted pipeline on the same inputs, with and without VitEngine(mid_gemm=True)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import boxes as ob
from oracle import vit as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME, NC, S, B = "vit_tiny_test", 5, 128, 2
FULL_KEYS = ("num_dets", "bboxes", "scores", "labels", "det_count", "crop_total")       # written in full by their kernels
LIVE_KEYS = ("det_box", "det_score", "det_label", "crop_rect", "crop_ok")                # (B, slots, ..): the first det_count[b] slots


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.fixture(scope="module")
def parts():
    """Engines, images, and a conf threshold under which the random-weight detector leaves 3 .. 16 crops (chosen from its own
    scores); the unfitted result and the fp32 oracle logits of its crops, computed once."""
    import yvhip
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    yvhip.require_gpu()
    ysd = engines.init_yolo_state("n", NC, seed=1, head_gain=4.0)
    vsd = engines.init_vit_wrapper_state(NAME, NC, seed=2)
    yolo = engines.YoloEngine(ysd, "n", NC, S, DEV)
    vit = engines.VitEngine(vsd, NAME, NC, device=DEV, mid_gemm=False)
    vit_mid = engines.VitEngine(vsd, NAME, NC, device=DEV, mid_gemm=True)
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    imgd = img.to(DEV)
    probe = DetectClassifyPipeline(yolo, [vit], conf=0.0).detect_stage(imgd)
    scores = sorted((float(probe["det_score"][b, k]) for b in range(B) for k in range(int(probe["det_count"][b]))), reverse=True)
    conf, base = None, None
    for keep in (8, 6, 12, 4, 16, 3):                  # a threshold between two neighbouring scores; dedupe may take some away
        if len(scores) <= keep or scores[keep - 1] == scores[keep]:
            continue
        c = 0.5 * (scores[keep - 1] + scores[keep])
        out = DetectClassifyPipeline(yolo, [vit], conf=c)(imgd)
        if 2 < int(out["crop_total"][0]) <= 16:
            conf, base = c, out
            break
    assert conf is not None, scores
    torch.cuda.synchronize()
    base = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in base.items()}
    total = int(base["crop_total"][0])
    ref = []
    for row in base["crop_list"][:total].tolist():
        x = torch.from_numpy(ob.crop_resize_normalize(img[row[0]].numpy(), row[1:5]))[None]
        ref.append(ov.wrapper_forward(vsd, x, NAME)[0])
    return dict(yolo=yolo, vit=vit, vit_mid=vit_mid, img=imgd, conf=conf, base=base, total=total, ref=torch.stack(ref), vsd=vsd)


def test_fit_crops_against_the_unfitted_pipeline(parts):
    import yvhip
    from yvhip.pipeline import DetectClassifyPipeline, fit_capacity
    base, total, ref = parts["base"], parts["total"], parts["ref"]
    assert 2 < total <= 16
    assert base["capacity"] == B * 100
    results = {"unfitted": base}
    for label, vit in (("fit_crops", parts["vit"]), ("fit_crops + mid_gemm", parts["vit_mid"])):
        out = DetectClassifyPipeline(parts["yolo"], [vit], conf=parts["conf"], fit_crops=True)(parts["img"])
        torch.cuda.synchronize()
        results[label] = out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
        for k in FULL_KEYS:
            assert torch.equal(out[k], base[k]), k
        for k in LIVE_KEYS:
            for b in range(B):
                n = int(base["det_count"][b])
                assert torch.equal(out[k][b, :n], base[k][b, :n]), (k, b)
        assert torch.equal(out["crop_list"][:total], base["crop_list"][:total])
        assert out["crop_list"].shape == base["crop_list"].shape                  # the list keeps its allocation
        assert out["capacity"] == fit_capacity(total, B * 100) == 1 << (total - 1).bit_length()
        assert out["cls_logits"].shape == (out["capacity"], NC) and out["cls_label"].shape == (out["capacity"],)
    assert yvhip.get_option("linear_mid") == 0                                   # restored after the mid_gemm pass
    for label, out in results.items():
        err = rel_l2(out["cls_logits"][:total], ref)
        print(f"{label}: rel-L2 of {total} crops' logits against the fp32 oracle {err:.3e}")
        assert err < 2e-2, label                                                 # the bound of tests/test_gpu_models.py
        assert out["cls_label"][:total].tolist() == out["cls_logits"][:total].argmax(1).tolist(), label


def test_mid_gemm_pass_takes_the_mid_route(parts):
    """The engine's block products at the fitted capacity are the mid-M route's under the option the pass sets, and the 128 x 128
    route's without it."""
    import yvhip
    from yvhip import engines
    from yvhip.pipeline import fit_capacity
    vit = parts["vit_mid"]
    M = fit_capacity(parts["total"], B * 100) * vit.N
    assert 256 < M <= engines.MID_GEMM_ROWS
    D = vit.D
    shapes = ((3 * D, D, 0), (D, D, yvhip.EPI_RES_F32), (4 * D, D, yvhip.EPI_GELU), (D, 4 * D, yvhip.EPI_RES_F32))
    old = yvhip.get_option("linear_mid")
    try:
        for n, k, f in shapes:
            assert yvhip.linear_route(M, n, k, f | yvhip.EPI_BIAS, m_dev=True).kernel == yvhip.LIN_DMA
        yvhip.set_option("linear_mid", engines.MID_GEMM_ROWS)
        for n, k, f in shapes:
            assert yvhip.linear_route(M, n, k, f | yvhip.EPI_BIAS, m_dev=True).kernel == yvhip.LIN_MID
    finally:
        yvhip.set_option("linear_mid", old)


def _count_classifier_launches(monkeypatch):
    """Counting wrappers around what a classifier pass launches first (the crop gather) and most (its linears)."""
    from yvhip import engines, pipeline
    calls = {"linear": 0, "layernorm": 0, "crop_resize_norm": 0}

    def counted(mod, name):
        real = getattr(mod, name)

        def f(*a, **kw):
            calls[name] += 1
            return real(*a, **kw)
        monkeypatch.setattr(mod, name, f)
    counted(engines, "linear")
    counted(engines, "layernorm")
    counted(pipeline, "crop_resize_norm")
    return calls


def test_zero_detections_launch_no_classifier(parts, monkeypatch):
    from yvhip.pipeline import DetectClassifyPipeline
    calls = _count_classifier_launches(monkeypatch)
    out = DetectClassifyPipeline(parts["yolo"], [parts["vit"]], conf=parts["conf"], fit_crops=True)(parts["img"])
    assert calls["linear"] > 0 and calls["crop_resize_norm"] == 1                # the counters see a pass ...
    for k in calls:
        calls[k] = 0
    out = DetectClassifyPipeline(parts["yolo"], [parts["vit"]], conf=2.0, fit_crops=True)(parts["img"])
    torch.cuda.synchronize()
    assert calls == {"linear": 0, "layernorm": 0, "crop_resize_norm": 0}         # ... and none where no score reaches conf
    assert int(out["crop_total"][0]) == 0 and out["capacity"] == 0
    assert out["cls_logits"].shape == (0, NC) and out["cls_logits"].dtype == torch.float32
    assert out["cls_label"].shape == (0,) and out["cls_label"].dtype == torch.int32


class _CFG:
    num_classes, device, modelName, pretrained = NC, DEV, NAME, None


def _main_parts(tmp_path, sizes):
    import utils.utils as uu
    from PIL import Image
    from YOLOTensorRT.models import TRTModule
    eng = TRTModule("random:n:5:1", torch.device(DEV), size=S)
    wpath = str(tmp_path / "best.pth")
    from yvhip import engines
    torch.save(engines.init_vit_wrapper_state(NAME, NC, seed=2), wpath)
    net = uu.build_model(CFG=_CFG, modelName=NAME, pretrained=wpath)
    net.to(DEV); net.eval()
    g = np.random.default_rng(5)
    (tmp_path / "im").mkdir()
    paths = []
    for i, (w, h) in enumerate(sizes):
        paths.append(str(tmp_path / "im" / f"img_{i}.png"))
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(paths[-1])
    return eng, net, paths


def test_main_zero_detections(tmp_path, monkeypatch):
    from YOLOTensorRT.inferdet import main
    eng, net, paths = _main_parts(tmp_path, [(128, 128)])
    eng.score_threshold = 2.0                                                    # no score reaches it: the NMS keeps nothing
    calls = _count_classifier_launches(monkeypatch)
    res = main(Engine=eng, imgs=paths[0], device=torch.device(DEV), model_list=[net], fit_crops=True)
    assert res == {"output": [{"image": os.path.basename(paths[0]), "objects": []}]}
    assert calls == {"linear": 0, "layernorm": 0, "crop_resize_norm": 0}


def test_main_fit_crops_against_main(tmp_path, monkeypatch):
    """Same objects, boxes, confidences and det_sort; `sort` equal wherever the unfitted run's top-2 logit margin exceeds twice
    the largest logit difference between the two runs."""
    from YOLOTensorRT import inferdet
    from YOLOTensorRT.config import CLASSES
    eng, net, paths = _main_parts(tmp_path, [(128, 128), (200, 150)])
    logits = []
    real = inferdet.DetectClassifyPipeline.__call__

    def keep(self, *a, **kw):
        out = real(self, *a, **kw)
        n = int(out["crop_total"][0])
        logits.append((out["crop_list"][:n].cpu(), out["cls_logits"][:n].cpu()))
        return out
    monkeypatch.setattr(inferdet.DetectClassifyPipeline, "__call__", keep)
    call = lambda **kw: inferdet.main(Engine=eng, imgs=str(tmp_path / "im"), device=torch.device(DEV), model_list=[net], **kw)
    r0, r1 = call(), call(fit_crops=True)
    monkeypatch.setenv("YV_FIT_CROPS", "1")
    r2 = call()                                                                  # the environment variable: the same switch
    assert r2 == r1
    (cl0, lg0), (cl1, lg1) = logits[0], logits[1]
    assert torch.equal(cl0, cl1) and lg0.shape == lg1.shape and lg0.shape[0] > 0
    diff = float((lg0 - lg1).abs().max())
    top2 = lg0.topk(2, 1).values
    sure = {(int(c[0]), int(c[5])) for c, m in zip(cl0, top2[:, 0] - top2[:, 1]) if float(m) > 2 * diff}
    assert [r["image"] for r in r0["output"]] == [r["image"] for r in r1["output"]]
    # objects of image i are its detections with a classified crop, in detection order: the same (image, k) keys in both runs
    keys = [[] for _ in paths]
    for c in cl0.tolist():
        keys[c[0]].append((c[0], c[5]))
    compared = 0
    names = sorted(os.path.basename(p) for p in paths)
    for i, p in enumerate(paths):
        o0 = r0["output"][names.index(os.path.basename(p))]["objects"]
        o1 = r1["output"][names.index(os.path.basename(p))]["objects"]
        assert len(o0) == len(o1) == len(keys[i])
        for a, b, key in zip(o0, o1, sorted(keys[i], key=lambda t: t[1])):
            assert {k: v for k, v in a.items() if k != "sort"} == {k: v for k, v in b.items() if k != "sort"}
            assert a["sort"] in CLASSES and b["sort"] in CLASSES
            if key in sure:
                assert a["sort"] == b["sort"]
                compared += 1
    assert compared > 0


def test_pipelined_runner_refuses_fit_crops(parts):
    import yvhip
    from yvhip.pipeline import DetectClassifyPipeline, PipelinedRunner
    pipe = DetectClassifyPipeline(parts["yolo"], [parts["vit"]], fit_crops=True)
    with pytest.raises(yvhip.YvError, match="fit_crops"):
        PipelinedRunner(pipe)
    PipelinedRunner(DetectClassifyPipeline(parts["yolo"], [parts["vit"]]))       # the default still constructs


def test_buffer_sets_stay_bounded(parts):
    """Totals 1, 3, 5, 3, 1 (injected crop counts) leave at most ceil(log2(cap)) + 2 capacities in the engine's buffer sets."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline, fit_capacity
    vit = engines.VitEngine(parts["vsd"], NAME, NC, device=DEV)
    pipe = DetectClassifyPipeline(parts["yolo"], [vit], conf=parts["conf"], fit_crops=True)
    cap = B * 100
    real = pipe.detect_stage
    want = []

    def inject(total):
        def stage(*a, **kw):
            det = real(*a, **kw)
            n = int(det["crop_total"][0])
            assert n >= 1
            # repeat the first crop: a list of `total` valid crops whatever the detector found
            det["crop_list"][:total] = det["crop_list"][:1].expand(total, -1)
            det["crop_total"].fill_(total)
            return det
        return stage
    for total in (1, 3, 5, 3, 1):
        pipe.detect_stage = inject(total)
        out = pipe(parts["img"])
        torch.cuda.synchronize()
        want.append(fit_capacity(total, cap))
        assert out["capacity"] == want[-1]
        lg = out["cls_logits"][:total].cpu()
        assert torch.equal(lg, lg[:1].expand(total, -1))                         # the same crop: the same logits in every row
    caps = {k[0] for k in vit._bufs}
    assert caps == set(want) == {1, 4, 8}
    assert len(caps) <= math.ceil(math.log2(cap)) + 2
