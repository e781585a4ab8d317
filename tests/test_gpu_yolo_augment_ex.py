"""GPU tests of `yv_mosaic_augment_ex` (csrc/augment.hip): bit equality with `yv_mosaic_augment` on affine records and with
the numpy statement (tests/yolo_augment_emulation.py) on drawn all-knob records and on degenerate ones, in-bounds writes,
the trainer's route through it, and labels that follow their objects under rotation."""
import numpy as np
import pytest
import torch

import yolo_augment_emulation as em

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def _tiles(S, n_tiles, seed):
    from yvhip.yolo_augment import tile_geometry
    rng = np.random.default_rng(seed)
    sizes = [tile_geometry(int(rng.integers(S // 3, 2 * S)), int(rng.integers(S // 3, 2 * S)), S) for _ in range(n_tiles)]
    tiles = np.full((n_tiles, S, S, 3), 114, np.uint8)
    for k, (w, h) in enumerate(sizes):
        tiles[k, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return tiles, sizes


def _batch_records(plans, sizes, S):
    """Records of a batch the way augment_batch packs them (tile k holds source k)."""
    from yvhip.yolo_augment import batch_records_ex
    return batch_records_ex(plans, dict(enumerate(sizes)), {k: k for k in range(len(sizes))}, S)


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(a).to(DEV) for a in arrays]


@pytest.mark.parametrize("S,B", [(50, 5), (64, 16)])
def test_affine_records_equal_the_old_entry_point(yv, S, B):
    """Single layer, last row (0, 0, 1): w is exactly 1 and the divide changes nothing.  2,500 pixels leave the last
    256-thread block partly filled."""
    from yvhip.yolo_augment import DetAugment, build_record
    n = 6
    tiles, sizes = _tiles(S, n, S)
    aug = DetAugment(S, seed=S)
    rf, ri, lut = [], [], []
    for b in range(B):
        p = aug.plan(b % n, n, use_mosaic=(b % 4 != 3))
        p["flip"] = bool(b & 1)                                                  # both values of bit 0, whatever the draw
        f, i, l, _, _, _ = build_record(p, [sizes[s] for s in p["sources"]], p["sources"], S)
        rf.append(f); ri.append(i); lut.append(l)
    rf, ri, lut = np.stack(rf), np.stack(ri), np.stack(lut)
    rec_h = np.concatenate([rf, np.tile(np.array([0, 0, 1], np.float32), (B, 1))], axis=1).reshape(B, 1, 9)
    t, f, i, l, h, i3 = _dev(tiles, rf, ri, lut, rec_h, ri.reshape(B, 1, 34))
    old = yv.mosaic_augment(t, f, i, l)
    new = yv.mosaic_augment_ex(t, h, i3, None, l)
    torch.cuda.synchronize()
    assert new.shape == (B, S, S, 3) and new.dtype == torch.uint8
    assert torch.equal(new, old)
    assert len({int(v) for v in ri[:, 1]}) == 2


@pytest.mark.parametrize("S,B", [(50, 5), (64, 16), (160, 3)])
def test_all_knobs_equal_the_emulation(yv, S, B):
    from yvhip.yolo_augment import DetAugment
    n = 6
    tiles, sizes = _tiles(S, n, S + 1)
    aug = DetAugment(S, seed=S + 2, degrees=45.0, shear=10.0, perspective=0.001, flipud=0.5, mixup=0.5)
    plans = [aug.plan(b % n, n) for b in range(B)]
    if B >= 5:                                                                   # the batch mixes two-layer and one-layer images
        plans[0].pop("mix", None)
        assert any(p.get("mix") for p in plans)
    plans[-1]["flipud"], plans[-1]["flip"] = True, True
    plans[0]["flipud"] = False
    rec_h, rec_i, mix, lut = _batch_records(plans, sizes, S)
    assert rec_h.shape[1] == 2 or B < 5
    out = yv.mosaic_augment_ex(*_dev(tiles, rec_h, rec_i, mix if rec_h.shape[1] == 2 else None, lut))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(out[b], em.apply_record_ex(tiles, rec_h[b], rec_i[b], mix[b], lut[b], S), err_msg=f"image {b}")


def test_degenerate_records_stay_in_bounds(yv):
    """Records come from the host: whatever they hold, the kernel reads inside `tiles`, writes inside `out` and shows the
    fill value where the emulation does."""
    from yvhip.yolo_augment import DetAugment
    S, B, n = 32, 8, 4
    tiles, sizes = _tiles(S, n, 9)
    aug = DetAugment(S, seed=10, degrees=20.0, mixup=1.0)
    rec_h, rec_i, mix, lut = _batch_records([aug.plan(b % n, n) for b in range(B)], sizes, S)
    assert rec_h.shape == (B, 2, 9)
    rec_h[0, 0] = (np.nan, 1e30, -1e30, np.inf, 0, 1, 0, 0, 1)
    rec_h[0, 1] = (1, 0, 0, 0, 1, 0, np.nan, np.inf, 1e30)
    rec_h[1, 0, 8] = -1.0                                                        # w <= 0 everywhere: layer 0 is all fill
    rec_h[1, 0, 6:8] = 0.0
    rec_h[2, :, 6:] = (0.1, -0.05, -0.5)                                         # w changes sign across the image
    rec_h[3, 1, 6:] = (0.0, 0.0, 0.0)                                            # w == 0
    mix[1], mix[4:7] = 1.0, (np.nan, -1.0, 2.0)
    rec_i[5, 1, 2::8] = (99, -5, 4, 7)                                           # layer 1 only: tile ids outside the tile array
    rec_i[6, 1, 0] = 1000                                                        # layer 1 only: tile count out of range
    rec_i[6, 1, 2:] = np.random.default_rng(0).integers(-200, 200, 32)
    rec_i[6, 1, 2::8] = (0, 1, 2, 3)
    rec_i[7, 0, 1] = 0x7FFFFFF3                                                  # only bits 0 and 1 of the flip word count
    lut[7] = np.random.default_rng(1).integers(0, 256, (3, 256), dtype=np.uint8)
    t, h, i, m, l = _dev(tiles, rec_h, rec_i, mix, lut)
    out = yv.mosaic_augment_ex(t, h, i, m, l)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(out[b], em.apply_record_ex(tiles, rec_h[b], rec_i[b], mix[b], lut[b], S), err_msg=f"image {b}")
    assert (out[1] == out[1][0, 0]).all()                                        # all fill, weight 1: one colour everywhere
    # a sentinel-padded output buffer, written through the C entry point: nothing outside `out` is touched
    import ctypes as C
    nbytes, pad = B * S * S * 3, 4096
    buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    yv.check(yv.lib.yv_mosaic_augment_ex(yv._p(t), n, B, S, 2, yv._p(h), yv._p(i), yv._p(m), yv._p(l),
                                         C.c_void_p(buf.data_ptr() + pad), yv._st()), "yv_mosaic_augment_ex")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:pad] == 0xA5).all() and (got[pad + nbytes:] == 0xA5).all()
    np.testing.assert_array_equal(got[pad:pad + nbytes].reshape(B, S, S, 3), out)


def test_wrapper_argument_checks(yv):
    S, B = 16, 2
    t = torch.zeros(1, S, S, 3, dtype=torch.uint8, device=DEV)
    h = torch.zeros(B, 2, 9, device=DEV)
    i = torch.zeros(B, 2, 34, dtype=torch.int32, device=DEV)
    m = torch.ones(B, device=DEV)
    l = torch.zeros(B, 3, 256, dtype=torch.uint8, device=DEV)
    assert yv.mosaic_augment_ex(t, h, i, m, l).shape == (B, S, S, 3)
    for bad, name in (((t[..., :2].contiguous(), h, i, m, l), "tiles"), ((t, h[:, :, :8].contiguous(), i, m, l), "rec_h"),
                      ((t, torch.zeros(B, 3, 9, device=DEV), i, m, l), "rec_h"), ((t, h, i[:1], m, l), "rec_i"),
                      ((t, h, i.float(), m, l), "rec_i"), ((t, h, i, None, l), "mix"), ((t, h, i, m[:1], l), "mix"),
                      ((t, h, i, m, l[:, :2].contiguous()), "lut")):
        with pytest.raises(yv.YvError, match=name):
            yv.mosaic_augment_ex(*bad)
    with pytest.raises(yv.YvError):
        yv.mosaic_augment_ex(t.cpu(), h, i, m, l)


def _surface_dataset(tmp_path):
    """The dataset recipe of test_train_yolo_surface: generate_annotation XML -> xml2pd -> images/labels tree -> data yaml."""
    import random as _r
    from PIL import Image
    from utils.class_config import xml2pd
    from utils.utils import generate_annotation
    rng = np.random.default_rng(0)
    src = tmp_path / "new"; src.mkdir()
    for i in range(6):
        img = rng.integers(90, 130, (96, 128, 3), dtype=np.uint8)
        x0, y0 = int(rng.integers(8, 60)), int(rng.integers(8, 40))
        img[y0:y0 + 40, x0:x0 + 48] = (220, 40, 40) if i % 2 else (40, 40, 220)
        Image.fromarray(img).save(src / f"im{i}.png")
        generate_annotation("new", f"im{i}.png", f"im{i}.png",
                            [{"sort": i % 2, "xmin": x0, "ymin": y0, "xmax": x0 + 48, "ymax": y0 + 40}], save_dir=str(src) + "/")
    _r.seed(3)
    root = tmp_path / "yolo" / "fold0"
    xml2pd(str(src), yolo_root=str(root))
    (tmp_path / "config.yaml").write_text(f"path: {root}\ntrain: images/train\nval: images/val\nnc: 5\n"
                                          "names: ['good', 'broke', 'lose', 'uncovered', 'circle']\n")
    return str(tmp_path / "config.yaml")


def test_trainer_run(yv, monkeypatch, tmp_path):
    import utils.trainYolo as ty
    data = _surface_dataset(tmp_path)
    calls = []
    real, real_ex = yv.mosaic_augment, yv.mosaic_augment_ex

    def spy(*a):
        calls.append("plain")
        return real(*a)

    def spy_ex(tiles, rec_h, rec_i, mix, lut):
        calls.append(("ex", rec_h.shape[1]))
        return real_ex(tiles, rec_h, rec_i, mix, lut)

    monkeypatch.setattr(yv, "mosaic_augment", spy)
    monkeypatch.setattr(yv, "mosaic_augment_ex", spy_ex)
    res = ty.train(epochs=2, batch=2, data=data, size=128, save=str(tmp_path / "w" / "best.pth"), log=lambda s: None,
                   close_mosaic=1, degrees=15, shear=2, perspective=0.0005, flipud=0.5, mixup=0.5)
    steps = res["epochs"][0]["steps"]
    assert len(res["epochs"]) == 2 and steps >= 1 and all(np.isfinite(e["loss"]) for e in res["epochs"])
    assert isinstance(res["not_built"], list) and any("copy-paste" in s for s in res["not_built"])
    assert not any(w in s for s in res["not_built"] for w in ("rotation", "shear", "perspective", "mixup"))
    assert len(calls) == 2 * steps
    assert all(c != "plain" for c in calls[:steps])                              # the open-mosaic epoch went through the new kernel
    assert all(c == "plain" or c == ("ex", 1) for c in calls[steps:])            # mosaic closed: no second layer any more
    calls.clear()
    res = ty.train(epochs=1, batch=2, data=data, size=128, save=str(tmp_path / "w" / "plain.pth"), log=lambda s: None)
    assert calls == ["plain"] * res["epochs"][0]["steps"] and calls


def test_labels_follow_objects_under_rotation(yv, tmp_path):
    """The bright-rectangle files of test_augment_batch_from_files with degrees 30 and HSV gains 0: the 3 x 3 neighbourhood
    at the centre of every returned box of at least 8 px is bright (mean > 200), because the hull of a rotated rectangle is
    centred on the rectangle.  That argument needs the whole hull: a box that the clip to [0, S] has cut (it touches the
    image border) is centred on what is left of the hull, which can lie beside the rectangle (on the numpy statement with
    this seed: 2 boxes of 21, both cut by the border, centre means 121.6 and 176.2).  Such a box must still hold bright
    pixels of its rectangle; the centre statement is asserted for every other one."""
    from PIL import Image
    from yvhip.yolo_augment import DetAugment, augment_batch
    S, n = 128, 5
    rng = np.random.default_rng(0)
    (tmp_path / "images").mkdir(); (tmp_path / "labels").mkdir()
    samples = []
    for i in range(n):
        w, h = int(rng.integers(90, 200)), int(rng.integers(90, 200))
        img = np.full((h, w, 3), 20, np.uint8)
        x0, y0, bw, bh = int(rng.integers(5, w // 2)), int(rng.integers(5, h // 2)), w // 3, h // 3
        img[y0:y0 + bh, x0:x0 + bw] = 235
        ip, lp = tmp_path / "images" / f"a{i}.png", tmp_path / "labels" / f"a{i}.txt"
        Image.fromarray(img).save(ip)
        lp.write_text(f"{i % 3} {(x0 + bw / 2) / w} {(y0 + bh / 2) / h} {bw / w} {bh / h}\n")
        samples.append((str(ip), str(lp)))
    aug = DetAugment(S, seed=4, degrees=30.0, hsv=(0.0, 0.0, 0.0))
    checked = 0
    for use_mosaic in (True, False, True):
        img, gtb, gtl, gtn = augment_batch(samples, range(4), aug, 8, DEV, use_mosaic=use_mosaic)
        assert img.shape == (4, S, S, 3) and img.dtype == torch.uint8 and img.is_cuda
        im = img.cpu().numpy().astype(np.float32).max(axis=3)
        for b in range(4):
            for j in range(int(gtn[b])):
                x1, y1, x2, y2 = gtb[b, j].tolist()
                assert 0 <= x1 < x2 <= S and 0 <= y1 < y2 <= S and 0 <= int(gtl[b, j]) < 3
                if x2 - x1 < 8 or y2 - y1 < 8:
                    continue
                if min(x1, y1) <= 0 or max(x2, y2) >= S:                         # cut by the clip: only part of the hull is left
                    assert im[b, int(y1):int(y2), int(x1):int(x2)].max() > 200, (use_mosaic, b, j, gtb[b, j])
                    continue
                cx, cy = int((x1 + x2) / 2), int((y1 + y2) / 2)
                assert im[b, cy - 1:cy + 2, cx - 1:cx + 2].mean() > 200, (use_mosaic, b, j, gtb[b, j])
                checked += 1
    assert checked >= 6, checked
