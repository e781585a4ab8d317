"""CPU: the host side of request sessions (yvhip.request, inferdet.main(graph=)) and the record reference the GPU tests use:
tests/request_reference.py against the loop of inferdet.main, the keys, the request block, yv_pack_results' argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import request_reference as rr
import yvhip
from yvhip import request


def _hand_case(cap):
    h = rr.hand_made()
    crop_list, total = rr.compact_ref(h["det_count"], h["crop_rect"], h["crop_ok"], cap)
    cls_label, cls_logits = rr.classifier_outputs(cap, h["nc"])
    words = rr.pack_ref(crop_list, [total], h["det_box"], h["det_score"], h["det_label"], cls_label, cls_logits, cap)
    return h, crop_list, total, cls_label, cls_logits, words


@pytest.mark.parametrize("cap", [4, 6, 3])
def test_records_give_the_objects_of_mains_loop(cap):
    """cap 4: total == cap; 6: zero rows past the total; 3: the list is cut at cap, as yv_compact_crops cuts it."""
    h, crop_list, total, cls_label, cls_logits, words = _hand_case(cap)
    assert total == min(4, cap) and words.shape == (1 + cap, 9 + h["nc"])
    assert words[0].tolist() == [total, h["B"], h["slots"], cap, h["nc"]] + [0] * (4 + h["nc"])
    assert not words[1 + total:].any()
    rec = request.unpack_results(words, h["nc"])
    want = rr.main_loop(h["det_count"], h["det_box"], h["det_score"], h["det_label"], crop_list, total, cls_label)
    assert rr.records_per_image(rec, h["B"]) == want
    assert [len(o) for o in want] == ([2, 0, 2] if cap >= 4 else [2, 0, 1])
    assert [o[0] for o in want[0]] == [0, 2]                        # the detection with crop_ok = 0 in the middle is skipped
    assert rec["score"].dtype == np.float32 and rec["logits"].dtype == np.float32 and rec["logits"].shape == (total, h["nc"])
    assert np.array_equal(rec["logits"], cls_logits[:total])
    assert request.unpack_results(words[:1 + total], h["nc"])["box"].tolist() == rec["box"].tolist()       # the first rows suffice


def test_records_give_mains_dict():
    """inferdet's two object builders - from the eager reads (main's loop, moved) and from the records - agree."""
    from YOLOTensorRT import inferdet
    h, crop_list, total, cls_label, cls_logits, words = _hand_case(4)
    cls_of = {(int(crop_list[k, 0]), int(crop_list[k, 5])): int(cls_label[k]) for k in range(total)}
    reads = inferdet._objects_of_reads(h["det_count"].tolist(), torch.from_numpy(h["det_box"]), torch.from_numpy(h["det_score"]),
                                       torch.from_numpy(h["det_label"]), cls_of)
    recs = inferdet._objects_of_records(request.unpack_results(words, h["nc"]), h["B"])
    assert reads == recs and [len(o) for o in recs] == [2, 0, 2]
    o = recs[2][1]
    assert o == {"sort": inferdet.CLASSES[int(cls_label[3])], "det_sort": inferdet.CLASSES[int(h["det_label"][2, 1]) % len(inferdet.CLASSES)],
                 "confidence": float(h["det_score"][2, 1]), "xmin": int(h["det_box"][2, 1, 0]), "ymin": int(h["det_box"][2, 1, 1]),
                 "xmax": int(h["det_box"][2, 1, 2]), "ymax": int(h["det_box"][2, 1, 3])}
    assert all(type(o[k]) is int for k in ("xmin", "ymin", "xmax", "ymax")) and type(o["confidence"]) is float


@pytest.mark.parametrize("total", [1, 2])
def test_unpack_results_owns_its_arrays(total):
    """A session hands in its pinned download buffer, which the next request overwrites: no returned array may be a view of it.
    One record is the case numpy would hand out as a view (a (1, nc) slice counts as contiguous)."""
    h = rr.hand_made()
    crop_list, _ = rr.compact_ref(h["det_count"], h["crop_rect"], h["crop_ok"], 4)
    cls_label, cls_logits = rr.classifier_outputs(4, h["nc"])
    words = rr.pack_ref(crop_list, [total], h["det_box"], h["det_score"], h["det_label"], cls_label, cls_logits, total)
    assert words.shape == (1 + total, 9 + h["nc"])
    rec = request.unpack_results(words, h["nc"])
    held = {k: v.copy() for k, v in rec.items()}
    assert not any(np.shares_memory(v, words) for v in rec.values())
    words[1:] = 0x5A5A5A5A
    for k, v in rec.items():
        assert v.tobytes() == held[k].tobytes(), k
    assert np.array_equal(rec["logits"], cls_logits[:total])


def test_frozen_state_names_what_a_capture_freezes():
    class _O:
        def __init__(self, names):
            for i, n in enumerate(names):
                setattr(self, n, i)
    pipe = _O(request.PIPE_FROZEN)
    pipe.yolo, pipe.vits = _O(request.YOLO_FROZEN), [_O(request.VIT_FROZEN), _O(request.VIT_FROZEN)]
    base = request.frozen_state(pipe)
    assert base == request.frozen_state(pipe)
    for obj, names in ((pipe, request.PIPE_FROZEN), (pipe.yolo, request.YOLO_FROZEN), (pipe.vits[1], request.VIT_FROZEN)):
        for n in names:
            old = getattr(obj, n)
            setattr(obj, n, -1)
            assert request.frozen_state(pipe) != base, n
            setattr(obj, n, old)
    assert {"conf", "dedupe_iou", "coord_mode", "max_crops"} <= set(request.PIPE_FROZEN)
    assert {"fused_c2f", "fused_tail"} <= set(request.YOLO_FROZEN) and "mid_gemm" in request.VIT_FROZEN


def test_unpack_results_rejects_other_buffers():
    h, _, _, _, _, words = _hand_case(4)
    for bad in (words.astype(np.int64), words[:, :-1], words.reshape(-1), words[:3]):
        with pytest.raises(yvhip.YvError):
            request.unpack_results(bad, h["nc"])
    with pytest.raises(yvhip.YvError):
        request.unpack_results(words, h["nc"] + 1)
    empty = request.empty_results(5)
    assert empty["image"].shape == (0,) and empty["box"].shape == (0, 4) and empty["logits"].shape == (0, 5)


def test_session_key_rounding():
    assert request.session_key(1, 640, 640) == (1, 640, 640)
    assert request.session_key(4, 641, 1) == (4, 704, 64)
    assert request.session_key(2, 64, 65) == (2, 64, 128)
    assert request.session_key(2, 100, 48) == request.session_key(2, 128, 64) == request.session_key(2, 65, 1) == (2, 128, 64)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        with pytest.raises(yvhip.YvError):
            request.session_key(*bad)


def test_request_block_layout():
    """{geom (B, 6) | ratio (B) | dwdh (2B) | wh (2B)}: the words of main's four uploads, floats by their bits."""
    from YOLOTensorRT.models.utils import letterbox_geometry
    shapes = [(100, 48), (48, 100), (64, 64)]
    B = len(shapes)
    lay = request.block_layout(B)
    assert lay == {"geom": (0, 18), "ratio": (18, 21), "dwdh": (21, 27), "wh": (27, 33), "words": (0, 33)}
    blk = request.request_block(shapes, (64, 96))
    assert blk.dtype == np.int32 and blk.shape == (33,)
    geom, ratio, dwdh, wh = [], [], [], []
    for h, w in shapes:
        r, (dw, dh), (nw, nh), (left, top) = letterbox_geometry(h, w, (64, 96))
        geom.append([w, h, nw, nh, left, top]); ratio.append(r); dwdh += [dw, dh]; wh += [w, h]
    assert blk[0:18].reshape(B, 6).tolist() == geom and blk[27:33].tolist() == wh
    # what torch.tensor(.., dtype=torch.float32) makes of main's Python floats
    assert np.array_equal(blk[18:21].view(np.float32), torch.tensor(ratio, dtype=torch.float32).numpy())
    assert np.array_equal(blk[21:27].view(np.float32), torch.tensor(dwdh, dtype=torch.float32).numpy())
    out = np.full(33, -1, dtype=np.int32)
    assert request.request_block(shapes, (64, 96), out=out) is out and np.array_equal(out, blk)
    with pytest.raises(yvhip.YvError):
        request.request_block(shapes, (64, 96), out=np.zeros(32, dtype=np.int32))


def test_images_that_fit_no_rule():
    ok = np.zeros((4, 5, 3), dtype=np.uint8)
    assert len(request.check_images([ok, ok])) == 2
    for bad in ([], None, [ok.astype(np.float32)], [ok[..., :2]], [ok[0]], [np.zeros((0, 5, 3), dtype=np.uint8)], [ok, "x"]):
        with pytest.raises(yvhip.YvError):
            request.check_images(bad)


def test_pack_results_argument_checks_without_gpu():
    """Decided on the host before any HIP call: null pointers, B, slots, nc <= 0, cap < 0."""
    fn = yvhip.lib.yv_pack_results
    p = ctypes.c_void_p(0x1000)                                        # never dereferenced: every call below is rejected first
    good = [p, p, p, p, p, p, p, 2, 4, 3, 5, p, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 11):
        args = list(good)
        args[i] = None
        assert fn(*args) == -1, i
    for i, v in ((7, 0), (7, -1), (8, 0), (9, -1), (10, 0), (10, -3)):
        args = list(good)
        args[i] = v
        assert fn(*args) == -1, (i, v)
    assert "yv_pack_results" in yvhip._SIGS and "yv_pack_results" in yvhip.header_symbols()


def test_main_graph_refuses_rect_before_touching_the_device(monkeypatch):
    from YOLOTensorRT import inferdet
    touched = []
    monkeypatch.setattr(yvhip, "require_gpu", lambda: touched.append(1))
    with pytest.raises(yvhip.YvError, match="rect"):
        inferdet.main(Engine=None, imgs=[], model_list=[object()], rect=True, graph=True)
    monkeypatch.setenv("YV_REQUEST_GRAPH", "1")
    with pytest.raises(yvhip.YvError, match="rect"):
        inferdet.main(Engine=None, imgs=[], model_list=[object()], rect=True)
    assert touched == []
