"""GPU: rectangular detector input, YoloEngine(size=(H, W)), through every layer: the _hw decode / fused tail / letterbox entry
points, the engine against the oracle, MXFP8, the detect + classify pipeline, inferdet.main(rect=True) and validate(rect=True).
Shapes are the smallest at which the code can still go wrong: both orientations, a P5 map of 3 pixels ((32, 96): a ragged
16-pixel group in the fused tail), a stride-4 map of 24 x 40 ((96, 160): partial fused-C2f tiles)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import boxes as ob
from oracle import pipeline as op
from oracle import yolo as oy
from rect_reference import decode_hw, n_anchors, split_raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    assert yvhip.lib.yv_device_is_gfx950() == 1
    return yvhip


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------ decode
@pytest.mark.parametrize("nc", [5, 80])
@pytest.mark.parametrize("H,W", [(64, 96), (96, 64), (32, 160)])
def test_detect_decode_hw_vs_reference(yv, H, W, nc):
    B, A = 2, n_anchors(H, W)
    raw = torch.randn(B, 64 + nc, A, generator=torch.Generator().manual_seed(4)) * 2
    eb, es = decode_hw(raw, nc, H, W)
    box_l, cls_l = split_raw(raw, nc, H, W)
    ld = (nc + 7) // 8 * 8
    pad = [torch.zeros(*c.shape[:3], ld) for c in cls_l]
    for p, c in zip(pad, cls_l):
        p[..., :nc] = c
    gb, gs = yv.detect_decode([b.to(DEV) for b in box_l], [p.to(DEV) for p in pad], (H, W), nc)
    assert tuple(gb.shape) == (B, A, 4) and tuple(gs.shape) == (B, A, nc)
    # the tolerance of test_detect_decode_vs_oracle: exp() implementations differ; coordinates are O(100) px
    assert torch.allclose(gb.cpu(), eb, atol=2e-3, rtol=1e-5)
    assert torch.allclose(gs.cpu(), es, atol=1e-6, rtol=1e-5)


def test_detect_decode_pair_of_a_square_is_the_int_call(yv):
    S, nc, B = 64, 5, 2
    raw = torch.randn(B, 64 + nc, n_anchors(S, S), generator=torch.Generator().manual_seed(5)) * 2
    box_l, cls_l = split_raw(raw, nc, S, S)
    pad = [torch.zeros(*c.shape[:3], 8) for c in cls_l]
    for p, c in zip(pad, cls_l):
        p[..., :nc] = c
    box_d, cls_d = [b.to(DEV) for b in box_l], [p.to(DEV) for p in pad]
    b0, s0 = yv.detect_decode(box_d, cls_d, S, nc)
    b1, s1 = yv.detect_decode(box_d, cls_d, (S, S), nc)
    assert torch.equal(b0, b1) and torch.equal(s0, s1)


# ------------------------------------------------------------------ fused tail
@pytest.mark.parametrize("scale,nc,hw,B", [("n", 5, (32, 96), 1), ("s", 5, (64, 96), 2), ("m", 3, (96, 64), 2),
                                           ("n", 16, (96, 160), 2), ("m", 16, (32, 96), 1), ("s", 16, (96, 160), 1)])
def test_fused_detect_tail_hw_is_bit_identical(yv, scale, nc, hw, B):
    """yv_detect_tail_hw against the unfused 1 x 1 convolutions + yv_detect_decode_hw on the same rectangle: the same bits, for
    c3 = 64 / 128 / 192, ragged last 16-pixel groups (3 P5 pixels at (32, 96)) and nc up to 16."""
    from yvhip import engines
    eng = engines.YoloEngine(engines.init_yolo_state(scale, nc, seed=3, head_gain=4.0), scale, nc, hw, DEV)
    assert eng.fused_tail and eng.hw == hw and eng.size == hw and eng.A == n_anchors(*hw)
    g = torch.Generator().manual_seed(hw[0] + nc)
    img = torch.randint(0, 256, (B, *hw, 3), generator=g, dtype=torch.uint8).to(DEV)
    boxes_f, scores_f = eng(img)
    eng.fused_tail = False
    boxes_u, scores_u = eng(img)
    torch.cuda.synchronize()
    assert tuple(boxes_f.shape) == (B, eng.A, 4) and tuple(scores_f.shape) == (B, eng.A, nc)
    assert torch.equal(boxes_f, boxes_u)
    assert torch.equal(scores_f, scores_u)
    assert float(scores_f.max()) > 0.3 and float(boxes_f.abs().max()) > 10          # a non-trivial head


# ------------------------------------------------------------------ letterbox
@pytest.mark.parametrize("H,W", [(64, 96), (96, 64)])
def test_letterbox_hw_vs_oracle(yv, H, W):
    """One batch, one canvas, images of different sizes: landscape, portrait, an exact fit (identity copy), an upscale, and a
    wide strip whose resized height is far below the window.  Bit-exact against oracle.boxes.letterbox_image(im, W, H)."""
    from YOLOTensorRT.models.utils import letterbox_geometry
    rng = np.random.default_rng(H)
    sizes = [(100, 200), (150, 70), (H, W), (20, 30), (9, 190)]              # (h, w)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    Hc, Wc = max(h for h, _ in sizes), max(w for _, w in sizes)
    canvas = np.zeros((len(imgs), Hc, Wc, 3), dtype=np.uint8)
    geom = []
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        canvas[i, :h, :w] = im
        r, dwdh, (nw, nh), (left, top) = letterbox_geometry(h, w, (W, H))
        r2, dwdh2, (nw2, nh2), (top2, _, left2, _) = ob.letterbox_params(h, w, W, H)
        assert (r, dwdh, nw, nh, left, top) == (r2, dwdh2, nw2, nh2, left2, top2)
        geom.append([w, h, nw, nh, left, top])
    out = yv.letterbox(torch.from_numpy(canvas).to(DEV), torch.tensor(geom, dtype=torch.int32, device=DEV), (H, W))
    assert tuple(out.shape) == (len(imgs), H, W, 3)
    out = out.cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i], ob.letterbox_image(im, W, H)), sizes[i]
    assert np.array_equal(out[2], imgs[2])                                  # the exact fit


def test_models_utils_letterbox_takes_a_rectangle(yv):
    from YOLOTensorRT.models.utils import letterbox
    im = np.random.default_rng(2).integers(0, 256, (50, 120, 3), dtype=np.uint8)
    out, r, dwdh = letterbox(im, (96, 64))                                   # (W, H)
    assert out.shape == (64, 96, 3) and np.array_equal(out, ob.letterbox_image(im, 96, 64))
    assert (r, dwdh) == ob.letterbox_params(50, 120, 96, 64)[:2]
    sq, _, _ = letterbox(im, (64, 64))
    assert np.array_equal(sq, ob.letterbox_image(im, 64, 64))


# ------------------------------------------------------------------ engine
@pytest.mark.parametrize("scale,nc,hw,B", [("n", 5, (64, 96), 2), ("n", 5, (96, 64), 2), ("n", 5, (96, 160), 2),
                                           ("s", 80, (32, 96), 1), ("m", 80, (64, 96), 1), ("n", 5, (384, 640), 1)])
def test_yolo_engine_hw_vs_oracle(yv, scale, nc, hw, B):
    """The checks and bounds of test_yolo_engine_vs_oracle on rectangles."""
    from yvhip import engines
    H, W = hw
    sd = oy.init_state(scale, nc, seed=7)
    img = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    raw, outs = oy.forward_raw(sd, oy.blob(img), scale, nc, return_feats=True)
    assert raw.shape[-1] == n_anchors(H, W)
    eng = engines.YoloEngine(sd, scale, nc, hw)
    box_l, cls_l = eng.forward_raw(img.to(DEV))
    torch.cuda.synchronize()
    bufs = eng._buffers(B)
    for idx in (0, 1, 2, 4, 6, 9, 12, 15, 18, 21):
        got = bufs["out"][idx].float().permute(0, 3, 1, 2).cpu()
        assert got.shape == outs[idx].shape, idx
        assert rel_l2(got, outs[idx]) < 2e-2, idx
    ebox, ecls = split_raw(raw, nc, H, W)
    for s in range(3):
        assert rel_l2(box_l[s].cpu(), ebox[s]) < 2e-2
        assert rel_l2(cls_l[s][..., :nc].cpu(), ecls[s]) < 2e-2
    eb, es = decode_hw(raw, nc, H, W)
    gb, gs = eng(img.to(DEV))
    assert rel_l2(gs.cpu(), es) < 2e-2
    assert float((gb.cpu() - eb).abs().max()) < 0.02 * max(H, W)       # pixels; DFL expectation of bf16 logits


def test_yolo_engine_square_pair_resized_and_wrong_extent(yv):
    from yvhip import engines
    sd = engines.init_yolo_state("n", 5, seed=3, head_gain=4.0)
    g = torch.Generator().manual_seed(6)
    # a square given as a pair is the square engine
    e_int, e_pair = engines.YoloEngine(sd, "n", 5, 128, DEV), engines.YoloEngine(sd, "n", 5, (128, 128), DEV)
    assert e_pair.size == 128 and e_pair.hw == (128, 128) and e_int.hw == (128, 128) and e_pair.A == e_int.A
    img = torch.randint(0, 256, (2, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    (b0, s0), (b1, s1) = e_int(img), e_pair(img)
    assert torch.equal(b0, b1) and torch.equal(s0, s1)
    # resized(): the bits of a freshly built engine, on the parent's weights
    fresh, sib = engines.YoloEngine(sd, "n", 5, (64, 96), DEV), e_int.resized((64, 96))
    assert sib.hw == (64, 96) and sib.size == (64, 96) and sib.A == n_anchors(64, 96) and e_int.hw == (128, 128)
    assert all(sib.w[k].data_ptr() == e_int.w[k].data_ptr() and sib.b[k].data_ptr() == e_int.b[k].data_ptr() for k in e_int.w)
    assert all(a.data_ptr() == b.data_ptr() for pa, pb in zip(sib._tail_operands, e_int._tail_operands) for a, b in zip(pa, pb))
    assert sib.guard is not e_int.guard and sib._bufs is not e_int._bufs
    rimg = torch.randint(0, 256, (2, 64, 96, 3), generator=g, dtype=torch.uint8).to(DEV)
    (b2, s2), (b3, s3) = fresh(rimg), sib(rimg)
    assert torch.equal(b2, b3) and torch.equal(s2, s3)
    (b4, s4) = e_int(img)                                              # the parent is untouched by its sibling's run
    assert torch.equal(b0, b4) and torch.equal(s0, s4)
    # a wrong input extent, a transposed one included
    for bad in ((2, 96, 64, 3), (2, 64, 64, 3), (2, 128, 128, 3)):
        with pytest.raises(yv.YvError):
            sib(torch.zeros(bad, dtype=torch.uint8, device=DEV))
    with pytest.raises(yv.YvError):
        engines.YoloEngine(sd, "n", 5, (100, 640), DEV)
    with pytest.raises(yv.YvError):
        e_int.resized((64, 100))


def test_yolo_engine_mxfp8_hw_tracks_bf16(yv):
    """YoloEngine(dtype="mxfp8", size=(96, 160)), scale m, against its bf16 engine: the gates tests/test_gpu_conv_mx.py applies to
    the square engine of that scale (logits rel-L2 max < 0.07, smallest per-anchor cosine >= 0.99).  resized() shares the
    quantised weights."""
    from yvhip import engines
    hw = (96, 160)
    sd = engines.init_yolo_state("m", 5, seed=7, head_gain=4.0)
    e16 = engines.YoloEngine(sd, "m", 5, hw, DEV)
    e8 = engines.YoloEngine(sd, "m", 5, hw, DEV, dtype="mxfp8")
    assert e8.mx_layers == engines.mx_conv_plan("m", 5) and len(e8.mx_layers) > 0
    img = torch.randint(0, 256, (2, *hw, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).to(DEV)
    b16, c16 = e16.forward_raw(img)
    b8, c8 = e8.forward_raw(img)
    torch.cuda.synchronize()
    rel_max, cos_min = 0.0, 1.0
    for part16, part8 in ((b16, b8), (c16, c8)):
        for a, b in zip(part16, part8):
            a, b = a.double().flatten(0, 2), b.double().flatten(0, 2)            # (anchors, channels)
            rel_max = max(rel_max, float((b - a).norm() / a.norm()))
            cos_min = min(cos_min, float(F.cosine_similarity(a, b, dim=1).min()))
    print(f"\nYOLOv8m mxfp8 vs bf16 at {hw}: logits rel-L2 max {rel_max:.4f} (gate 0.07), per-anchor cosine min {cos_min:.5f} "
          f"(gate 0.99)")
    assert rel_max < 0.07 and cos_min >= 0.99
    sib = engines.YoloEngine(sd, "m", 5, 64, DEV, dtype="mxfp8").resized(hw)
    assert all(sib.wq[k][0].data_ptr() != 0 for k in sib.wq) and sorted(sib.wq) == sorted(e8.wq)
    bs, cs = sib.forward_raw(img)
    assert all(torch.equal(a, b) for a, b in zip(bs + cs, b8 + c8))


# ------------------------------------------------------------------ pipeline
def _letterboxed(yv, imgs, hw):
    """Sources (list of (h,w,3) u8 arrays) in one canvas -> src, net_in (device letterbox to hw), ratio, dwdh, wh lists."""
    from YOLOTensorRT.models.utils import letterbox_geometry
    H, W = hw
    Hc, Wc = max(a.shape[0] for a in imgs), max(a.shape[1] for a in imgs)
    canvas = np.zeros((len(imgs), Hc, Wc, 3), dtype=np.uint8)
    geom, ratio, dwdh, wh = [], [], [], []
    for i, a in enumerate(imgs):
        h, w = a.shape[:2]
        canvas[i, :h, :w] = a
        r, (dw, dh), (nw, nh), (left, top) = letterbox_geometry(h, w, (W, H))
        geom.append([w, h, nw, nh, left, top]); ratio.append(r); dwdh += [dw, dh]; wh += [w, h]
    src = torch.from_numpy(canvas).to(DEV)
    net_in = yv.letterbox(src, torch.tensor(geom, dtype=torch.int32, device=DEV), hw)
    return src, net_in, ratio, dwdh, wh


def test_pipeline_on_a_rectangle(yv):
    """B = 2 at a (96, 160) network input letterboxed from larger sources: the integer stages bit-exact against
    oracle.pipeline.post_stages fed with the device's own NMS outputs and that letterbox's ratio / dwdh / (w, h); the crops
    bit-exact against oracle.boxes.crop_resize_normalize from the sources."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    name, hw, R = "vit_tiny_test", (96, 160), 3
    ysd = engines.init_yolo_state("n", 5, seed=1, head_gain=4.0)
    vsd = engines.init_vit_wrapper_state(name, 5, seed=2)
    pipe = DetectClassifyPipeline(engines.YoloEngine(ysd, "n", 5, hw, DEV), [engines.VitEngine(vsd, name, 5, device=DEV)],
                                  max_crops_per_image=R)
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((150, 300), (200, 260))]
    src, net_in, ratio, dwdh, wh = _letterboxed(yv, imgs, hw)
    assert tuple(net_in.shape) == (2, 96, 160, 3)
    out = pipe(net_in, torch.tensor(ratio, dtype=torch.float32, device=DEV), torch.tensor(dwdh, dtype=torch.float32, device=DEV),
               torch.tensor(wh, dtype=torch.int32, device=DEV), src_images=src)
    crops = yv.crop_resize_norm(src, out["crop_list"], out["crop_total"], out["capacity"], 224, 16, layout=0).cpu()
    torch.cuda.synchronize()
    out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    assert int(out["det_count"].sum()) > 0
    n_crops = 0
    for b in range(2):
        dets = op.post_stages(out["num_dets"][b, 0], out["bboxes"][b], out["scores"][b], out["labels"][b],
                              float(np.float32(ratio[b])), (dwdh[2 * b], dwdh[2 * b + 1]), (wh[2 * b], wh[2 * b + 1]), max_crops=R)
        assert int(out["det_count"][b]) == len(dets)
        for k, d in enumerate(dets):
            assert out["det_box"][b, k].tolist() == d["box"] and out["crop_rect"][b, k].tolist() == d["rect"]
            if d["ok"]:
                assert out["crop_list"][n_crops].tolist() == [b] + d["rect"] + [k]
                assert np.array_equal(crops[n_crops].numpy(), ob.crop_resize_normalize(imgs[b], d["rect"]))
                n_crops += 1
    assert int(out["crop_total"][0]) == n_crops and n_crops > 0
    # without geometry the network input is its own source: (W, H) of the rectangle
    ident = pipe._identity_geometry(2, 96, 160, torch.device(DEV))
    assert ident["wh"].tolist() == [160, 96, 160, 96]


class _CFG:
    num_classes, device, modelName, pretrained = 5, DEV, "vit_tiny_test", None


def _cell_detector_state(nc: int = 5):
    """A YOLOv8n state dict that marks bright stride-8 cells: every convolution hands channel 0 on through its centre tap (the
    neck's model.15 takes it from the stride-8 skip), the stem maps red 114 (the letterbox fill) to 0 and red 255 to 11, and the
    P3 head answers with class 0 at logit ch0 - 6 and the DFL distance 0.5 on every side: the box of a cell whose top-left pixel
    is bright is that cell, nothing fires on the fill or on a dark pixel, and the coarser scales never fire.  So where the
    boxes land is known from the picture - random weights put boxes anywhere, also outside the picture."""
    from yvhip import engines
    sd = {}
    for key, ci, co, k in engines.yolo_conv_keys("n", nc):
        w, b = torch.zeros(co, ci, k, k), torch.zeros(co)
        src = engines._c(512, "n") if key == "model.15.cv1.conv" else 0       # concat (out12 | out4): the skip's channel 0
        w[0, src, k // 2, k // 2] = 1.0
        sd[key + ".weight"], sd[key + ".bias"] = w, b
    sd["model.0.conv.weight"][0, 0, 1, 1] = 20.0
    sd["model.0.conv.bias"][0] = -20.0 * 114 / 255
    for s in range(3):
        sd[f"model.22.cv2.{s}.2.weight"].zero_()
        sd[f"model.22.cv2.{s}.2.bias"].view(4, 16)[:, :2] = 30.0            # bins 0 and 1 alike: distance 0.5 cells
        sd[f"model.22.cv3.{s}.2.bias"].fill_(-20.0)
    sd["model.22.cv3.0.2.bias"][0] = -6.0
    sd["model.22.dfl.conv.weight"] = torch.arange(16, dtype=torch.float32).view(1, 16, 1, 1)
    return sd


def _block_image(h, w, y0, y1, x0, x1):
    """The fill value everywhere, a white block inside: the cells of _cell_detector_state that fire start inside the block."""
    im = np.full((h, w, 3), 114, dtype=np.uint8)
    im[y0:y1, x0:x1] = 255
    return im


def test_main_rect(yv, tmp_path):
    """inferdet.main(rect=True): every reported box inside its image; the objects those of a manual pipeline call on the same
    letterboxed batch.  The three files together need a 64 x 64 input; the landscape file alone runs at (32, 64).  The detector
    is _cell_detector_state: a box is a stride-8 cell (12.5 source pixels at ratio 0.64) that starts inside the white block, and
    every block ends at least 14 pixels before the right and bottom edges of its picture."""
    import utils.utils as uu
    from PIL import Image
    from YOLOTensorRT.config import CLASSES
    from YOLOTensorRT.inferdet import main
    from YOLOTensorRT.models import TRTModule
    from YOLOTensorRT.models.utils import rect_net_shape
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    assert TRTModule("random:n:5:1", torch.device(DEV), size=(64, 96)).inp_info[0].shape == (1, 3, 64, 96)
    S = 64
    eng = TRTModule(_cell_detector_state(), torch.device(DEV), size=S)
    assert eng.inp_info[0].shape == (1, 3, 64, 64) and eng.size == 64
    wpath = str(tmp_path / "best.pth")
    torch.save(engines.init_vit_wrapper_state("vit_tiny_test", 5, seed=2), wpath)
    net = uu.build_model(CFG=_CFG, modelName="vit_tiny_test", pretrained=wpath)
    net.to(DEV); net.eval()
    (tmp_path / "im").mkdir()
    paths = []
    pictures = [_block_image(100, 48, 30, 70, 12, 34), _block_image(48, 100, 8, 30, 20, 70), _block_image(64, 64, 16, 44, 16, 44)]
    for i, im in enumerate(pictures):                                   # 48 x 100, 100 x 48 and 64 x 64 (w x h)
        paths.append(str(tmp_path / "im" / f"img_{i}.png"))
        Image.fromarray(im).save(paths[-1])
    total = 0
    for chunk, want_hw in ((paths, (64, 64)), ([paths[1]], (32, 64))):
        res = main(Engine=eng, imgs=chunk if len(chunk) == 1 else str(tmp_path / "im"), device=torch.device(DEV),
                   model_list=[net], rect=True)
        assert [r["image"] for r in res["output"]] == [os.path.basename(p) for p in chunk]
        imgs = [np.asarray(Image.open(p).convert("RGB")) for p in chunk]
        hw = rect_net_shape([a.shape[:2] for a in imgs], S)
        assert hw == want_hw
        src, net_in, ratio, dwdh, wh = _letterboxed(yv, imgs, hw)
        pipe = DetectClassifyPipeline(eng.engine.resized(hw), [net.engine()], eng.score_threshold, eng.iou_threshold, eng.topk)
        out = pipe(net_in, torch.tensor(ratio, dtype=torch.float32, device=DEV), torch.tensor(dwdh, dtype=torch.float32, device=DEV),
                   torch.tensor(wh, dtype=torch.int32, device=DEV), src_images=src)
        out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
        ctot = int(out["crop_total"][0])
        cls_of = {(int(out["crop_list"][k, 0]), int(out["crop_list"][k, 5])): int(out["cls_label"][k]) for k in range(ctot)}
        for i, (r_, a) in enumerate(zip(res["output"], imgs)):
            h, w = a.shape[:2]
            want = []
            for k in range(int(out["det_count"][i])):
                if (i, k) in cls_of:
                    want.append((CLASSES[cls_of[(i, k)]], float(out["det_score"][i, k]), *out["det_box"][i, k].tolist()))
            got = [(o["sort"], o["confidence"], o["xmin"], o["ymin"], o["xmax"], o["ymax"]) for o in r_["objects"]]
            assert got == want
            for o in r_["objects"]:
                assert 0 <= o["xmin"] <= o["xmax"] <= w and 0 <= o["ymin"] <= o["ymax"] <= h, (o, w, h)
            assert len(got) > 0
            total += len(got)
    assert total > 0
    with pytest.raises(yv.YvError):
        main(Engine=TRTModule("random:n:5:1", torch.device(DEV), size=(64, 96)), imgs=paths, device=torch.device(DEV),
             model_list=[net], rect=True)


def test_validate_rect(yv, tmp_path):
    """validate(rect=True) on a five-image set at size 64: the batches run at the extents rect_batches gives, and the image
    and instance counts are those of the square walk.  (Metric parity is unpinned, as for the rest of validate.)"""
    from PIL import Image
    from yvhip.yolo_data import rect_batches
    from yvhip.yolo_training import init_yolo_train_state
    from yvhip.yolo_val import validate
    rng = np.random.default_rng(3)
    root = tmp_path / "d"
    (root / "images" / "val").mkdir(parents=True); (root / "labels" / "val").mkdir(parents=True)
    hw = [(96, 128), (128, 96), (64, 64), (50, 120), (120, 50)]
    samples = []
    for i, (h, w) in enumerate(hw):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "images" / "val" / f"v{i}.png")
        (root / "labels" / "val" / f"v{i}.txt").write_text(f"{i % 5} 0.5 0.5 0.4 0.5\n" * (1 + i % 2))
        samples.append((str(root / "images" / "val" / f"v{i}.png"), str(root / "labels" / "val" / f"v{i}.txt")))
    sd = init_yolo_train_state("n", 5, seed=1)
    for k in sd:
        if ".cv3." in k and k.endswith(".2.bias"):
            sd[k] = sd[k] + 6.0                         # random head but confident: plenty of candidates above conf
    plan = rect_batches(hw, 2, 64)
    assert [s for _, s in plan] == [(64, 96), (96, 96), (96, 64)]      # ratios .42 .75 | 1 1.33 | 2.4
    rect = validate(sd, samples, "n", 5, size=64, batch=2, conf=0.25, iou=0.6, rect=True)
    square = validate(sd, samples, "n", 5, size=64, batch=2, conf=0.25, iou=0.6)
    assert rect["shapes"] == [s for _, s in plan]
    assert square["shapes"] == [(64, 64)] * 3
    assert rect["images"] == square["images"] == 5 and rect["instances"] == square["instances"] == 7
    assert rect["detections"] > 0 and 0.0 <= rect["map50_95"] <= rect["map50"] <= 0.995
    none = validate(sd, [], "n", 5, size=64, rect=True)
    assert none["images"] == 0 and none["shapes"] == []
