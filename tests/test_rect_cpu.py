"""Rectangular detector input, the parts that need no GPU: the reference decode with separate extents, the host helpers that
choose the rectangles (rect_net_shape, rect_batches), label mapping into a rectangle, and the host-side argument checks of the
three _hw entry points."""
import ctypes

import numpy as np
import pytest
import torch

import yvhip
from oracle import boxes as ob
from oracle import yolo as oy
from rect_reference import decode_hw, make_anchors_hw, n_anchors


@pytest.mark.parametrize("size", [64, 128])
def test_decode_hw_equals_oracle_at_squares(size):
    nc = 5
    A = n_anchors(size, size)
    raw = torch.randn(2, 64 + nc, A, generator=torch.Generator().manual_seed(size)) * 2
    eb, es = oy.decode(raw, nc, size)
    gb, gs = decode_hw(raw, nc, size, size)
    assert torch.equal(gb, eb) and torch.equal(gs, es)
    a, s = make_anchors_hw(size, size)
    ea, es_ = oy.make_anchors(size)
    assert torch.equal(a, ea) and torch.equal(s, es_)


def test_anchor_order_of_a_rectangle():
    """(32, 96): 4 x 12 + 2 x 6 + 1 x 3 anchors; x runs fastest inside a scale."""
    a, s = make_anchors_hw(32, 96)
    assert a.shape == (48 + 12 + 3, 2) and n_anchors(32, 96) == 63 and yvhip.n_anchors(32, 96) == 63
    assert a[0].tolist() == [0.5, 0.5] and a[11].tolist() == [11.5, 0.5] and a[12].tolist() == [0.5, 1.5]
    assert a[48].tolist() == [0.5, 0.5] and a[60].tolist() == [0.5, 0.5] and a[62].tolist() == [2.5, 0.5]
    assert s[47] == 8 and s[48] == 16 and s[60] == 32


def test_rect_net_shape_hand_cases():
    from YOLOTensorRT.models.utils import rect_net_shape
    assert rect_net_shape([(1080, 1920)], 640) == (384, 640)          # r = 1/3: 360 x 640 -> 384 x 640
    assert rect_net_shape([(1920, 1080)], 640) == (640, 384)
    assert rect_net_shape([(1080, 1920), (1920, 1080)], 640) == (640, 640)      # a mixed chunk needs both long sides
    assert rect_net_shape([(480, 640), (1080, 1920)], 640) == (480, 640)        # 480 x 640 and 360 x 640
    assert rect_net_shape([(640, 640)], 640) == (640, 640)            # already S x S
    assert rect_net_shape([(100, 48)], 64) == (64, 32)                # r = 0.64: 64 x 31 (30.72 rounds up) -> 64 x 32
    assert rect_net_shape([(48, 100), (100, 48), (64, 64)], 64) == (64, 64)


def test_rect_batches_hand_cases():
    from yvhip.yolo_data import rect_batches
    assert rect_batches([(640, 640)], 16, 640) == [([0], (672, 672))]           # ceil(20 + 0.5) * 32, as upstream
    # 16:9 landscape: [0.5625, 1] -> ceil(11.25 + 0.5) = 12, ceil(20.5) = 21
    assert rect_batches([(1080, 1920)] * 3, 16, 640) == [([0, 1, 2], (384, 672))]
    # portrait: [1, 1 / 1.7778] -> 21, ceil(11.25 + 0.5) = 12
    assert rect_batches([(1920, 1080)], 16, 640) == [([0], (672, 384))]
    # a batch that straddles aspect ratio 1 stays square
    assert rect_batches([(1080, 1920), (1920, 1080)], 2, 640) == [([0, 1], (672, 672))]
    # sorted by h / w, then cut: ratios 1.78, 1, 0.5625, 0.75 -> [2, 3] (max 0.75: ceil(15.5) = 16) and [1, 0] (1 is not > 1)
    shapes = [(1920, 1080), (640, 640), (1080, 1920), (480, 640)]
    assert rect_batches(shapes, 2, 640) == [([2, 3], (512, 672)), ([1, 0], (672, 672))]
    assert rect_batches(shapes, 2, 64) == [([2, 3], (64, 96)), ([1, 0], (96, 96))]
    assert rect_batches([], 4, 640) == []


def test_load_batch_maps_labels_into_the_rectangle(tmp_path):
    from PIL import Image
    from yvhip.yolo_data import letterbox_host, load_batch
    h, w, H, W = 40, 80, 64, 96
    rng = np.random.default_rng(1)
    ip, lp = str(tmp_path / "a.png"), str(tmp_path / "a.txt")
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(ip)
    open(lp, "w").write("1 0.5 0.5 0.5 0.5\n")
    img, gtb, gtl, gtn = load_batch([(ip, lp)], (H, W), 2)
    r, _, (nw, nh), (top, _, left, _) = ob.letterbox_params(h, w, W, H)
    assert (r, nw, nh, top, left) == (1.2, 96, 48, 8, 0)              # by hand: min(64/40, 96/80); pads (0, 8)
    assert tuple(img.shape) == (1, H, W, 3) and int(gtn[0]) == 1 and int(gtl[0, 0]) == 1
    want = np.float32([20 * r + left, 10 * r + top, 60 * r + left, 30 * r + top])
    assert np.array_equal(gtb[0, 0].numpy(), want) and want.tolist() == [24.0, 20.0, 72.0, 44.0]
    assert bool((img[0, :top] == 114).all()) and bool((img[0, top + nh:] == 114).all())
    # the square form is the pair form with H = W
    a, ra, pa = letterbox_host(np.asarray(Image.open(ip)), 64)
    b, rb, pb = letterbox_host(np.asarray(Image.open(ip)), (64, 64))
    assert np.array_equal(a, b) and ra == rb and pa == pb


def test_hw_entry_points_check_arguments_on_the_host():
    """Host-only checks, before any HIP call: null pointers, a side that is no multiple of 32, a side <= 0."""
    lib = yvhip.lib
    p = 4096                                                          # a non-null value that is never dereferenced
    arr = (ctypes.c_void_p * 3)(p, p, p)
    dec = lambda H, W, box0=p, out=p: lib.yv_detect_decode_hw(box0, p, p, p, p, p, 8, 1, H, W, 5, out, p, None)
    tail = lambda H, W, f0=p, w2=arr: lib.yv_detect_tail_hw(f0, p, p, 128, 64, w2, arr, arr, arr, 1, H, W, 5, p, p, None)
    lbx = lambda H, W, src=p, out=p: lib.yv_letterbox_hw(src, 1, 10, 10, p, H, W, out, None)
    for fn in (dec, tail, lbx):
        assert fn(100, 64) == -1 and fn(64, 100) == -1                # not multiples of 32
        assert fn(64, 0) == -1 and fn(0, 64) == -1 and fn(-32, 64) == -1
        assert fn(64, 96, None) == -1                                 # null first pointer
    assert dec(64, 96, p, None) == -1 and lbx(64, 96, p, None) == -1 and tail(64, 96, p, None) == -1
    assert lib.yv_detect_decode_hw(p, p, p, p, p, p, 4, 1, 64, 96, 5, p, p, None) == -1          # cls_ld < nc, as the square form
    assert lib.yv_detect_tail_hw(p, p, p, 128, 64, arr, arr, arr, arr, 1, 64, 96, 17, p, p, None) == -1     # nc > 16


def test_engine_size_check_needs_no_gpu():
    from yvhip import engines
    assert engines.net_hw is yvhip.net_hw
    assert yvhip.net_hw(640) == (640, 640) and yvhip.net_hw((384, 640)) == (384, 640) and yvhip.net_hw([64, 96]) == (64, 96)
    for bad in ((100, 640), (640, 100), 100, (0, 64), (64, 96, 3)):
        with pytest.raises(yvhip.YvError):
            yvhip.net_hw(bad)
