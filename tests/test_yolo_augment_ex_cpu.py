"""CPU tests of the detector augmentation's non-default knobs (degrees, shear, perspective, flipud, mixup): the numpy
statement of `yv_mosaic_augment_ex` (tests/yolo_augment_emulation.py) anchored to the committed oracle, the conventions of
the forward matrix, that image and labels move together, the plan's draw order and the host-side argument errors.
No GPU, no compute calls into the library."""
import ctypes as C

import numpy as np
import pytest

import yolo_augment_emulation as em
from oracle import yolo_augment as oy

ALL_ON = dict(degrees=30.0, shear=5.0, perspective=0.0005)


def _tiles(sizes, S, seed=0, grey=False):
    rng = np.random.default_rng(seed)
    tiles = np.full((len(sizes), S, S, 3), 114, dtype=np.uint8)
    for k, (w, h) in enumerate(sizes):
        px = rng.integers(0, 256, (h, w, 1 if grey else 3), dtype=np.uint8)
        tiles[k, :h, :w] = px
    return tiles


def _sizes(n, S, seed):
    from yvhip.yolo_augment import tile_geometry
    rng = np.random.default_rng(seed)
    return [tile_geometry(int(rng.integers(S // 3, 2 * S)), int(rng.integers(S // 3, 2 * S)), S) for _ in range(n)]


def _record_ex(plan, sizes, S):
    from yvhip.yolo_augment import build_record_ex, plan_layers
    layers = plan_layers(plan)
    return build_record_ex(plan, [[sizes[s] for s in l["sources"]] for l in layers], [l["sources"] for l in layers], S)


# ------------------------------------------------------------------------------------------------ emulation vs oracle
@pytest.mark.parametrize("S", [32, 64])
def test_emulation_is_anchored_to_the_oracle(S):
    from yvhip.yolo_augment import DetAugment, build_record
    n = 6
    sizes = _sizes(n, S, S)
    tiles = _tiles(sizes, S, S)
    aug = DetAugment(S, seed=S)
    for b in range(8):
        p = aug.plan(b % n, n, use_mosaic=(b % 4 != 3))
        rec_f, rec_i, lut, _, _, _ = build_record(p, [sizes[s] for s in p["sources"]], p["sources"], S)
        rec_h, rec_i2, mix, lut2, _, _, _ = _record_ex(p, sizes, S)
        assert rec_h.shape == (1, 9) and mix == 1.0
        np.testing.assert_array_equal(rec_i2[0], rec_i)
        np.testing.assert_array_equal(lut2, lut)
        np.testing.assert_array_equal(em.apply_record_ex(tiles, rec_h, rec_i2, None, lut, S),
                                      oy.apply_record(tiles, rec_f, rec_i, lut, S), err_msg=f"plan {b}")


def test_zero_knobs_change_nothing():
    from yvhip.yolo_augment import DetAugment, affine_matrix, build_record, forward_matrix, plan_is_default
    S, n = 64, 7
    sizes = _sizes(n, S, 1)
    a, b = DetAugment(S, seed=3), DetAugment(S, seed=3, degrees=0, shear=0, perspective=0, flipud=0, mixup=0)
    for k in range(200):
        pa, pb = a.plan(k % n, n, k % 5 != 0), b.plan(k % n, n, k % 5 != 0)
        assert pa == pb and plan_is_default(pa)
        assert set(pa) <= {"mosaic", "sources", "centre", "scale", "translate", "hsv", "flip"}     # today's keys, nothing new
        rec_f, rec_i, lut, M, _, canvas = build_record(pa, [sizes[s] for s in pa["sources"]], pa["sources"], S)
        rec_h, rec_i2, _, _, Ms, _, _ = _record_ex(pa, sizes, S)
        assert rec_h[0, :6].tobytes() == rec_f.tobytes()
        assert rec_h[0, 6:].tobytes() == np.array([0, 0, 1], np.float32).tobytes()
        assert rec_i2[0].tobytes() == rec_i.tobytes()
        assert Ms[0].tobytes() == M.tobytes()
        assert forward_matrix(canvas, S, pa["scale"], *pa["translate"]).tobytes() == \
            affine_matrix(canvas, S, pa["scale"], *pa["translate"]).tobytes()


# ------------------------------------------------------------------------------------------------ conventions
def _single_tile_plan(**kw):
    p = dict(mosaic=False, sources=[0], scale=1.0, translate=(0.5, 0.5), hsv=[1.0, 1.0, 1.0], flip=False)
    p.update(kw)
    return p


def _emulate(plan, tiles, sizes, S):
    rec_h, rec_i, mix, lut, _, _, _ = _record_ex(plan, sizes, S)
    return em.apply_record_ex(tiles, rec_h, rec_i, mix, lut, S)


def test_rotation_sense_and_centre():
    """A positive angle turns the picture counter-clockwise about the canvas point (S/2, S/2): half a pixel off the pixel
    grid's centre, so a quarter turn lands one row (one column) off np.rot90 and the vacated line shows the fill."""
    S = 16
    tiles = _tiles([(S, S)], S, 2, grey=True)
    out = _emulate(_single_tile_plan(angle=90.0), tiles, [(S, S)], S)
    np.testing.assert_array_equal(out[1:], np.rot90(tiles[0])[:-1])
    assert (out[0] == 114).all()
    out = _emulate(_single_tile_plan(angle=-90.0), tiles, [(S, S)], S)
    np.testing.assert_array_equal(out[:, 1:], np.rot90(tiles[0], -1)[:, :-1])
    assert (out[:, 0] == 114).all()
    for kw in (dict(angle=90.0), dict(angle=25.0, shear=(3.0, -2.0), perspective=(0.0004, -0.0003)), dict(flip=True)):
        plain, ud = _emulate(_single_tile_plan(**kw), tiles, [(S, S)], S), _emulate(_single_tile_plan(flipud=True, **kw), tiles, [(S, S)], S)
        np.testing.assert_array_equal(ud, plain[::-1])


def test_image_and_labels_use_the_same_matrix():
    """A peaked 3 x 3 blob planted at a known canvas point shows up where M (with the divide and the flips) sends the point,
    and the transformed box around it contains that point."""
    from yvhip.yolo_augment import DetAugment, build_record_ex, plan_labels
    S = 64
    sizes = [(S, S)] * 4
    checked = 0
    for seed in range(40):
        base = DetAugment(S, seed=seed, **ALL_ON).plan(0, 4)
        assert base["mosaic"] and {"angle", "shear", "perspective"} <= set(base)
        base.update(sources=[0, 1, 2, 3], hsv=[1.0, 1.0, 1.0])
        for flip, flipud in ((False, False), (True, False), (False, True), (True, True)):
            plan = dict(base, flip=flip, flipud=flipud)
            rec_h, rec_i, mix, lut, Ms, offs, _ = build_record_ex(plan, [sizes], [plan["sources"]], S)
            xc, yc = plan["centre"]
            q = np.array([xc - 9.0, yc - 9.0])                                   # canvas point, inside quadrant 0
            tx, ty = int(q[0]) - offs[0][0][0], int(q[1]) - offs[0][0][1]        # its tile pixel
            assert 1 <= tx < S - 1 and 1 <= ty < S - 1
            tiles = np.full((4, S, S, 3), 20, np.uint8)
            tiles[0, ty - 1:ty + 2, tx - 1:tx + 2] = 200
            tiles[0, ty, tx] = 255
            ph = Ms[0] @ [q[0], q[1], 1.0]
            if ph[2] <= 0:
                continue
            pt = ph[:2] / ph[2]
            if flip:
                pt[0] = S - 1 - pt[0]
            if flipud:
                pt[1] = S - 1 - pt[1]
            if not (10 <= pt[0] <= S - 11 and 10 <= pt[1] <= S - 11):            # the point leaves the image (or its margin)
                continue
            out = em.apply_record_ex(tiles, rec_h, rec_i, mix, lut, S).astype(np.int32).sum(axis=2)
            by, bx = np.unravel_index(np.argmax(out), out.shape)
            assert np.hypot(bx - pt[0], by - pt[1]) <= 1.5, (seed, flip, flipud, (bx, by), pt)
            labs = {0: np.array([[2, (tx + 0.5) / S, (ty + 0.5) / S, 12.0 / S, 12.0 / S]]), 1: np.zeros((0, 5)),
                    2: np.zeros((0, 5)), 3: np.zeros((0, 5))}
            nb, nl = plan_labels(plan, labs, {s: (S, S) for s in range(4)}, S)
            assert nl.tolist() == [2], (seed, flip, flipud)
            x1, y1, x2, y2 = nb[0]
            assert x1 <= pt[0] <= x2 and y1 <= pt[1] <= y2, (seed, flip, flipud, nb[0], pt)
            checked += 1
    assert checked >= 20, checked


# ------------------------------------------------------------------------------------------------ labels
def _transform_boxes_parent(boxes, labels, M, scale, S, flip):
    """The affine expression of `transform_boxes` as it stood before the perspective branch, restated to pin its bits."""
    b = boxes.astype(np.float64)
    corners = np.stack([b[:, [0, 1]], b[:, [2, 3]], b[:, [0, 3]], b[:, [2, 1]]], axis=1)
    pts = corners @ M[:2, :2].T + M[:2, 2]
    new = np.concatenate([pts.min(1), pts.max(1)], axis=1)
    new = np.clip(new, 0, S)
    w1, h1 = (b[:, 2] - b[:, 0]) * scale, (b[:, 3] - b[:, 1]) * scale
    w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
    eps = 1e-16
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    keep = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + eps) > 0.1) & (ar < 100)
    new, lab = new[keep], labels[keep]
    if flip:
        new = np.stack([S - new[:, 2], new[:, 1], S - new[:, 0], new[:, 3]], axis=1)
    return new.astype(np.float32), lab.astype(np.int32)


def test_perspective_labels():
    from yvhip.yolo_augment import affine_matrix, forward_matrix, homography_record, transform_boxes
    S = 64
    boxes = np.array([[40, 40, 60, 70], [0, 0, 33, 33], [90, 90, 128, 128], [50, 50, 51.5, 80], [20, 60, 100, 64.5]], float)
    labels = np.arange(5)
    # corners round-trip through M and the f32 record
    rng = np.random.default_rng(0)
    for _ in range(50):
        M = forward_matrix(2 * S, S, rng.uniform(0.5, 1.5), rng.uniform(0.4, 0.6), rng.uniform(0.4, 0.6), rng.uniform(-45, 45),
                           rng.uniform(-10, 10, 2), rng.uniform(-0.001, 0.001, 2))
        H = homography_record(M).astype(np.float64).reshape(3, 3)
        assert H[2, 2] == 1.0
        pts = rng.uniform(0, 2 * S, (8, 2))
        fw = np.c_[pts, np.ones(8)] @ M.T
        assert (fw[:, 2] > 0).all()
        out = fw[:, :2] / fw[:, 2:]
        back = np.c_[out, np.ones(8)] @ H.T
        np.testing.assert_allclose(back[:, :2] / back[:, 2:], pts, atol=1e-3, rtol=0)
    # a corner at w <= 0 drops the box
    M = np.eye(3)
    M[2, 0] = -0.01                                                             # w = 1 - x / 100
    nb, nl = transform_boxes(np.array([[10, 10, 50, 50], [90, 10, 100, 50], [90, 10, 120, 50]], float), np.arange(3), M, 1.0, 10 ** 6,
                             flip=False)
    assert nl.tolist() == [0]
    np.testing.assert_allclose(nb[0], [10 / 0.9, 10 / 0.9, 100.0, 100.0])
    # the affine branch keeps its bits
    for (scale, flip) in ((1.0, False), (1.0, True), (0.5, False), (0.73, True)):
        M = affine_matrix(2 * S, S, scale, 0.5, 0.47)
        got, want = transform_boxes(boxes, labels, M, scale, S, flip=flip), _transform_boxes_parent(boxes, labels, M, scale, S, flip)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and len(got[1]) > 0
    fu, _ = transform_boxes(boxes[:1], labels[:1], affine_matrix(2 * S, S, 1.0, 0.5, 0.5), 1.0, S, flip=False, flipud=True)
    np.testing.assert_allclose(fu[0], [8, 64 - 38, 28, 64 - 8])


# ------------------------------------------------------------------------------------------------ mixup
def test_mixup_plan_and_labels():
    from yvhip.yolo_augment import DetAugment, plan_is_default, plan_labels, plan_layers
    S, n = 64, 5
    aug = DetAugment(S, seed=8, mixup=1.0, **ALL_ON)
    firsts = set()
    rng = np.random.default_rng(1)
    sizes = {s: sz for s, sz in enumerate(_sizes(n, S, 4))}
    labs = {s: np.c_[rng.integers(0, 3, 3), rng.uniform(0.3, 0.7, (3, 2)), rng.uniform(0.2, 0.5, (3, 2))] for s in range(n)}
    concatenated = 0
    for k in range(100):
        p = aug.plan(k % n, n)
        assert p["mosaic"] and not plan_is_default(p) and len(plan_layers(p)) == 2 and 0.0 < p["mix_ratio"] < 1.0
        m = p["mix"]
        assert m["mosaic"] and len(m["sources"]) == 4 and all(0 <= s < n for s in m["sources"]) and "centre" in m
        assert {"angle", "shear", "perspective", "scale", "translate"} <= set(m) and "hsv" not in m and "flip" not in m
        assert (m["scale"], m["angle"], m["centre"]) != (p["scale"], p["angle"], p["centre"])
        firsts.add(m["sources"][0])
        shared = dict(hsv=p["hsv"], flip=p["flip"], flipud=p.get("flipud", False))
        b0, l0 = plan_labels({k2: v for k2, v in p.items() if k2 not in ("mix", "mix_ratio")}, labs, sizes, S)
        b1, l1 = plan_labels(dict(m, **shared), labs, sizes, S)
        bb, ll = plan_labels(p, labs, sizes, S)
        np.testing.assert_array_equal(bb, np.concatenate([b0, b1]))
        np.testing.assert_array_equal(ll, np.concatenate([l0, l1]))
        concatenated += len(l0) > 0 and len(l1) > 0
    assert firsts == set(range(n)) and concatenated >= 50
    ratios = [aug.plan(0, n)["mix_ratio"] for _ in range(400)]
    assert abs(np.mean(ratios) - 0.5) < 0.02 and 0.04 < np.std(ratios) < 0.08                       # Beta(32, 32): sd 0.062
    for k in range(50):
        assert "mix" not in aug.plan(k % n, n, use_mosaic=False)
    half = DetAugment(S, seed=9, mixup=0.5)
    taken = sum("mix" in half.plan(k % n, n) for k in range(1000))
    assert abs(taken / 1000 - 0.5) < 0.05


def test_draw_order_and_ranges():
    """A non-zero knob draws between the existing draws, in the order of RandomPerspective.affine_transform: the stream of
    a reference generator read in that order reproduces the plan."""
    from yvhip.yolo_augment import DetAugment
    S, n = 64, 9
    aug = DetAugment(S, seed=21, degrees=40.0, shear=7.0, perspective=0.0008, flipud=0.3)
    r = np.random.default_rng(21)
    ups = 0
    for k in range(300):
        p = aug.plan(k % n, n)
        assert r.random() < 1.0                                                  # mosaic
        assert p["sources"][1:] == [int(v) for v in r.integers(0, n, 3)]
        assert p["centre"] == (int(r.uniform(S / 2, 3 * S / 2)), int(r.uniform(S / 2, 3 * S / 2)))
        assert p["perspective"] == (float(r.uniform(-0.0008, 0.0008)), float(r.uniform(-0.0008, 0.0008)))
        assert p["angle"] == float(r.uniform(-40.0, 40.0))
        assert p["scale"] == float(r.uniform(0.5, 1.5))
        assert p["shear"] == (float(r.uniform(-7.0, 7.0)), float(r.uniform(-7.0, 7.0)))
        assert p["translate"] == (float(r.uniform(0.4, 0.6)), float(r.uniform(0.4, 0.6)))
        assert p["flipud"] == bool(r.random() < 0.3)
        assert p["hsv"] == [float(v) for v in r.uniform(-1, 1, 3) * np.asarray((0.015, 0.7, 0.4)) + 1]
        assert p["flip"] == bool(r.random() < 0.5)
        assert abs(p["angle"]) <= 40 and all(abs(v) <= 7 for v in p["shear"]) and all(abs(v) <= 0.0008 for v in p["perspective"])
        ups += p["flipud"]
    assert abs(ups / 300 - 0.3) < 0.08


def test_emulated_blend():
    from yvhip.yolo_augment import hsv_tables
    S = 8
    tiles = np.stack([np.full((S, S, 3), 200, np.uint8), np.full((S, S, 3), 100, np.uint8)])
    rec_h = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32), (2, 1))
    rec_i = np.zeros((2, 34), np.int32)
    rec_i[0, 0], rec_i[0, 2:9] = 1, (0, 0, 0, S, S, 0, 0)
    rec_i[1, 0], rec_i[1, 2:9] = 1, (1, 0, 0, S, S, 0, 0)
    lut = hsv_tables([1, 1, 1])
    assert (em.apply_record_ex(tiles, rec_h, rec_i, 0.25, lut, S) == 125).all()
    f = np.float32
    m = f(0.3)
    want = np.floor(f(f(m * f(200)) + f(f(f(1) - m) * f(100))))                # the stated f32 arithmetic, one rounding per step
    assert want == 130.0
    assert (em.apply_record_ex(tiles, rec_h, rec_i, 0.3, lut, S) == int(want)).all()
    # a weight whose exact blend lies just under a whole number truncates: 0.7 * 200 + 0.3 * 100 = 170 - 2.4e-6 in f32 steps
    m = f(0.7)
    want = np.floor(f(f(m * f(200)) + f(f(f(1) - m) * f(100))))
    assert (em.apply_record_ex(tiles, rec_h, rec_i, 0.7, lut, S) == int(want)).all()
    for mix, v in ((np.nan, 100), (-1.0, 100), (2.0, 200), (1.0, 200), (0.0, 100)):
        assert (em.apply_record_ex(tiles, rec_h, rec_i, mix, lut, S) == v).all(), mix
    rec_h[1, 8] = -1.0                                                          # w <= 0: layer 1 is the fill value
    assert (em.apply_record_ex(tiles, rec_h, rec_i, 0.5, lut, S) == 157).all()


# ------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("kw", [dict(degrees=-1), dict(degrees=181), dict(shear=-0.1), dict(shear=89), dict(perspective=-1e-4),
                                dict(perspective=0.0011), dict(flipud=-0.1), dict(flipud=1.1), dict(mixup=-0.1), dict(mixup=1.5),
                                dict(degrees=float("nan"))])
def test_range_errors(kw):
    import yvhip
    from yvhip.yolo_augment import DetAugment
    with pytest.raises(yvhip.YvError, match=next(iter(kw))):
        DetAugment(64, seed=0, **kw)


def test_range_limits_are_accepted():
    from yvhip.yolo_augment import DetAugment
    DetAugment(64, seed=0, degrees=180, shear=88.9, perspective=0.001, flipud=1, mixup=1)


def test_train_argument_errors(tmp_path):
    import yvhip
    import utils.trainYolo as ty
    with pytest.raises(yvhip.YvError, match="copy_paste.*mask"):
        ty.train(epochs=1, batch=1, data=str(tmp_path / "none.yaml"), copy_paste=0.1)
    with pytest.raises(yvhip.YvError, match="degrees"):
        ty.train(epochs=1, batch=1, data=str(tmp_path / "none.yaml"), degrees=200)
    assert len(ty.NOT_BUILT) == 1 and "copy-paste" in ty.NOT_BUILT[0]
    assert not any(w in ty.NOT_BUILT[0] for w in ("rotation", "shear", "perspective", "mixup"))


def test_ex_argument_validation_without_gpu():
    """Argument errors of yv_mosaic_augment_ex are detected on the host before any HIP call."""
    import yvhip
    fn = yvhip.lib.yv_mosaic_augment_ex
    buf = C.create_string_buffer(4096)                                          # never dereferenced: every call below is refused
    p = C.cast(buf, C.c_void_p)
    assert fn(None, 1, 1, 8, 1, None, None, None, None, None, None) == -1
    for k in (0, 5, 6, 8, 9):                                                   # tiles, rec_h, rec_i, lut, out
        args = [p, 1, 1, 8, 1, p, p, p, p, p, None]
        args[k] = None
        assert fn(*args) == -1, k
    assert fn(p, 1, 1, 8, 0, p, p, p, p, p, None) == -1
    assert fn(p, 1, 1, 8, 3, p, p, p, p, p, None) == -1
    assert fn(p, 1, 1, 8, 2, p, p, None, p, p, None) == -1
    assert fn(p, 1, 0, 8, 1, p, p, None, p, p, None) == 0                       # B == 0: nothing to do
    assert fn(p, 1, 0, 8, 2, p, p, p, p, p, None) == 0
