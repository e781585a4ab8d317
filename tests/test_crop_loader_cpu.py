"""CPU checks of the device-resident crop loader (yvhip/crop_loader.py, utils.trainClass.build_dataloader(device_pool=...)):
the plan the device loader builds is the host loader's batch (same samples, rectangles, labels, paths, RNG consumption),
the pool round-trips every image and decodes it once, the cap raises, and the default path is what it was."""
import random

import numpy as np
import pytest
import torch

import crop_loader_emulation as em
from oracle import boxes as ob


@pytest.fixture()
def tc(monkeypatch):
    import utils.trainClass as tc
    monkeypatch.setattr(tc.CFG, "train_bs", 5, raising=False)
    monkeypatch.setattr(tc.CFG, "valid_bs", 3, raising=False)
    return tc


def _objects(tc, tmp_path, seed):
    random.seed(seed)
    tr = tc.xml2pd([em.write_dataset(tmp_path / "tr", seed=1, n_images=7)])
    va = tc.xml2pd([em.write_dataset(tmp_path / "va", seed=2, n_images=4, many=3)])
    return tr, va


def _host_pool(objs_lists):
    from yvhip.crop_loader import DevicePool
    return DevicePool([o["path"] for lst in objs_lists for o in lst], device=None)


def _apply(batch, S):
    pool = batch.pool
    return np.stack([ob.crop_resize_normalize(pool.image(int(r[0])), r[1:5], (S, S)) for r in batch.plan])


@pytest.mark.parametrize("seed", [3, 17])
def test_plan_equals_host_batches(tc, tmp_path, seed):
    (objs, circ), (vobjs, vcirc) = _objects(tc, tmp_path, 0)
    n = len(objs) + len(circ)
    assert n % tc.CFG.train_bs != 0 and len(circ) >= 2          # a short last batch and a live circle switch
    pool = _host_pool([objs, circ, vobjs, vcirc])
    S = tc.CFG.img_size[0]
    got = {}
    for kind in ("host", "device"):
        tc.set_seed(seed)
        tf = tc.build_transforms(tc.CFG)
        loaders = tc.build_dataloader(objs, circ, vobjs, vcirc, tf, **({"device_pool": pool} if kind == "device" else {}))
        rec = []
        for loader in loaders:                                   # train epoch, then validation, like fit()
            for inputs, targets, paths in loader:
                x = inputs.numpy() if kind == "host" else _apply(inputs, S)
                assert tuple(inputs.shape) == x.shape
                rec.append((x, targets.numpy(), list(paths)))
        # the records train_one_epoch would draw next come from a generator seeded from `random` at build_transforms
        got[kind] = (rec, random.getstate(), np.random.get_state()[1].tolist(), torch.random.get_rng_state().tolist(),
                     tf["train"].device_augment.sample(2))
    (hrec, hr, hn, ht, haug), (drec, dr, dn, dt, daug) = got["host"], got["device"]
    assert len(hrec) == len(drec) == -(-n // 5) + -(-(len(vobjs) + len(vcirc)) // 3)
    assert hrec[-(-n // 5) - 1][0].shape[0] == n % 5             # the short last training batch is there
    for k, ((hx, hy, hp), (dx, dy, dp)) in enumerate(zip(hrec, drec)):
        assert hp == dp, k
        np.testing.assert_array_equal(hy, dy, err_msg=f"batch {k}")
        assert hx.dtype == dx.dtype == np.float32
        np.testing.assert_array_equal(hx.view(np.uint32), dx.view(np.uint32), err_msg=f"batch {k}")
    assert hr == dr and hn == dn and ht == dt
    np.testing.assert_array_equal(haug[0], daug[0])
    np.testing.assert_array_equal(haug[1], daug[1])


def test_emulated_tables_are_the_oracle_tables():
    """The numpy statement the GPU tests compare against folds the crop into the record's tables; for rectangles inside the
    image that is x0 + nearest_index_table(S, w)[mapx] (crops smaller and larger than S, drawn and edge records)."""
    from yvhip.augment import TrainAugment, identity_record, make_record
    table = np.array([[0, 700, 500], [700 * 500 * 3, 40, 30]], dtype=np.int64)
    for S in (64, 224):
        recs = [identity_record(S)[1], make_record(S, flip=True, crop_xy=(0, 0) if S >= 200 else None)[1]]
        recs += list(TrainAugment(S, seed=2).sample(6)[1])
        for img, rect in ((0, (3, 5, 640, 470)), (0, (100, 100, 101, 131)), (1, (0, 0, 40, 30)), (1, (7, 2, 20, 3)), (0, (0, 0, S, S))):
            for idx in recs:
                off, W, col, row = em.folded_tables(table, np.array([img, *rect]), idx, S)
                x0, y0, x1, y1 = rect
                assert (off, W) == (int(table[img, 0]), int(table[img, 1]))
                np.testing.assert_array_equal(col, x0 + ob.nearest_index_table(S, x1 - x0)[idx[36:36 + S]])
                np.testing.assert_array_equal(row, y0 + ob.nearest_index_table(S, y1 - y0)[idx[36 + S:]])
    # and the virtual crop is the oracle's crop
    rng = np.random.default_rng(0)
    pool = rng.integers(0, 256, int(table[1, 0]) + 40 * 30 * 3, dtype=np.uint8)
    img0 = pool[:700 * 500 * 3].reshape(500, 700, 3)
    for rect in ((3, 5, 640, 470), (100, 100, 101, 131), (0, 0, 700, 500)):
        np.testing.assert_array_equal(em.virtual_crop(pool, table, np.array([0, *rect]), 64), ob.crop_resize_normalize(img0, rect, (64, 64)))


def test_pool_round_trip_single_decode_and_cap(tc, tmp_path, monkeypatch):
    from PIL import Image
    from yvhip import YvError, crop_loader
    (objs, circ), _ = _objects(tc, tmp_path, 0)
    paths = [o["path"] for o in objs + circ]
    assert len(paths) > len(set(paths)) >= 7                     # several objects per image
    decodes = []
    real = crop_loader._decode
    monkeypatch.setattr(crop_loader, "_decode", lambda p: (decodes.append(p), real(p))[1])
    pool = crop_loader.DevicePool(paths, device=None)
    assert sorted(decodes) == sorted(set(paths)) and len(pool) == len(set(paths))
    total = 0
    for i, p in enumerate(pool.paths):
        want = np.asarray(Image.open(p).convert('RGB'))
        np.testing.assert_array_equal(pool.image(i), want)
        assert pool.sizes[i] == (want.shape[1], want.shape[0]) and pool.image_id(p) == i
        assert pool.host_table[i].tolist() == [total, want.shape[1], want.shape[0]]
        total += want.size
    assert pool.nbytes == total == pool.host_pool.size and pool.host_pool.dtype == np.uint8
    with pytest.raises(YvError, match=str(total)):
        crop_loader.DevicePool(paths, device=None, max_bytes=total - 1)
    crop_loader.DevicePool(paths, device=None, max_bytes=total)
    with pytest.raises(YvError, match="not in the pool"):
        pool.image_id("nowhere.png")
    assert crop_loader.DEFAULT_POOL_BYTES == 32 << 30


def test_degenerate_rectangle_names_file_and_box(tc, tmp_path):
    from yvhip import YvError
    (objs, circ), (vobjs, vcirc) = _objects(tc, tmp_path, 0)
    bad = dict(objs[0], objects=dict(objs[0]["objects"], xmin=10 ** 6, xmax=10 ** 6 + 4))       # right of the image
    pool = _host_pool([objs, circ])
    _, valid = tc.build_dataloader(objs, circ, [bad], [], tc.build_transforms(tc.CFG), device_pool=pool)
    with pytest.raises(YvError) as e:
        list(valid)
    assert bad["path"] in str(e.value) and str(10 ** 6 + 4) in str(e.value)


def test_default_loaders_unchanged(tc, tmp_path, monkeypatch):
    (objs, circ), (vobjs, vcirc) = _objects(tc, tmp_path, 0)
    tf = tc.build_transforms(tc.CFG)
    tr, va = tc.build_dataloader(objs, circ, vobjs, vcirc, tf)
    for ld, t in ((tr, tf["train"]), (va, tf["valid_test"])):
        assert type(ld) is torch.utils.data.DataLoader and type(ld.dataset) is tc.build_dataset and ld.dataset.transforms is t
    assert isinstance(tr.sampler, torch.utils.data.RandomSampler) and isinstance(va.sampler, torch.utils.data.SequentialSampler)
    assert type(tf["train"]) is tc._TrainTransform and type(tf["valid_test"]) is tc._EvalTransform
    # train() without CFG.device_loader asks for exactly those; with it, for the device loaders
    seen = []

    class Stop(Exception):
        pass

    def spy(*a, **k):
        seen.append(k)
        raise Stop

    monkeypatch.setattr(tc, "build_dataloader", spy)

    class C(tc.CFG):
        train_path, valid_path = [str(tmp_path / "tr")], [str(tmp_path / "va")]

    with pytest.raises(Stop):
        tc.train(C)

    class D(C):
        device_loader = True

    with pytest.raises(Stop):
        tc.train(D)
    assert [bool(k.get("device_pool", False)) for k in seen] == [False, True]


def test_wrapper_is_bound():
    import yvhip
    assert "yv_train_crops" in yvhip._SIGS and "yv_train_crops" in yvhip.header_symbols() and callable(yvhip.train_crops)
