"""GPU parity of `yv_train_crops` (csrc/train_crops.hip) and of the device-resident crop loader built on it: bit-exact
against oracle.boxes.crop_resize_normalize -> oracle.augment.apply_record, against the present two-step device path, and
end to end against the host loader of utils.trainClass."""
import json
import os
import random

import numpy as np
import pytest
import torch

import crop_loader_emulation as em
from oracle import augment as oa
from oracle import boxes as ob

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def _pool(sizes, seed):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    nb = [im.size for im in imgs]
    table = np.zeros((len(imgs), 3), dtype=np.int64)
    table[:, 0] = np.concatenate([[0], np.cumsum(nb)[:-1]])
    table[:, 1:] = sizes
    return imgs, np.concatenate([im.reshape(-1) for im in imgs]), table


def _run(yv, pool, table, plan, geo, idx, S, P, layout=2):
    out = yv.train_crops(*(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (pool, table, plan, geo, idx)), S, P, layout)
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


SIZES = [(640, 360), (97, 61), (33, 300), (256, 256), (1, 1)]


def _rects(S):
    """(image, x0, y0, x1, y1): upsampling, downsampling, 1 pixel wide / high, whole image, every border, a 1 x 1 image."""
    return [(0, 0, 0, 640, 360), (0, 100, 50, 600, 340), (0, 0, 17, 31, 40), (0, 630, 0, 640, 360), (0, 5, 350, 400, 360),
            (1, 0, 0, 97, 61), (1, 40, 20, 41, 60), (1, 3, 30, 90, 31), (1, 96, 60, 97, 61), (2, 0, 0, 33, 300),
            (2, 10, 100, 20, 290), (3, 0, 0, 256, 256), (3, 16, 16, 16 + S, 16 + S), (3, 200, 1, 256, 255), (4, 0, 0, 1, 1)]


def _all_at_once(S, rng):
    from yvhip.augment import make_record
    return [
        make_record(S, flip=True, crop_xy=(24, 24), ssr=(10.0, 1.05, 0.0625, -0.0625), perm=(2, 0, 1),
                    grid=(1 + rng.uniform(-.05, .05, 6), 1 + rng.uniform(-.05, .05, 6)),
                    holes=[(0, 0, 11, 11), (213, 213, 224, 224), (5, 100, 16, 111), (100, 5, 111, 16), (60, 60, 71, 71)]),
        make_record(S, flip=False, crop_xy=(0, 0), ssr=(-10.0, 0.95, -0.0625, 0.0625), elastic=rng.uniform(-50, 50, (3, 2)),
                    holes=[(i * 20, i * 25, i * 20 + 11, i * 25 + 11) for i in range(8)]),
        make_record(S, elastic=np.full((3, 2), 50.0)),
        make_record(S, ssr=(0.0, 1.0, 0.0, 0.0)),
    ]


def _records(S, n, seed):
    """n records: drawn ones, then (S = 224) every transform at once, then identity."""
    from yvhip.augment import TrainAugment, identity_record
    fixed = (_all_at_once(S, np.random.default_rng(5)) if S == 224 else []) + [identity_record(S)]
    geo, idx = TrainAugment(S, seed=seed).sample(n - len(fixed))
    assert (idx[:, 3] > 0).any() and (np.abs(geo[:, 0] - 1) > 1e-3).any()          # the draw exercises holes and warps
    return np.concatenate([geo, np.stack([r[0] for r in fixed])]), np.concatenate([idx, np.stack([r[1] for r in fixed])])


@pytest.mark.parametrize("S,P", [(224, 16), (224, 8), (64, 32)])
def test_kernel_matches_the_oracle_composition(yv, S, P):
    imgs, pool, table = _pool(SIZES, seed=S + P)
    plan = np.array(_rects(S), dtype=np.int32)
    geo, idx = _records(S, len(plan), seed=11)
    got = _run(yv, pool, table, plan, geo, idx, S, P)
    g2 = (S // P) ** 2
    for b, r in enumerate(plan):
        x = ob.crop_resize_normalize(imgs[r[0]], r[1:5], (S, S))
        np.testing.assert_array_equal(got[b * g2:(b + 1) * g2], oa.apply_record(x, geo[b], idx[b], P), err_msg=f"sample {b} {r}")
    # layout 0, identity records: the normalised crop itself
    from yvhip.augment import identity_record
    gi, ii = identity_record(S)
    f32 = _run(yv, pool, table, plan, np.stack([gi] * len(plan)), np.stack([ii] * len(plan)), S, 0, layout=0)
    for b, r in enumerate(plan):
        np.testing.assert_array_equal(f32[b], ob.crop_resize_normalize(imgs[r[0]], r[1:5], (S, S)), err_msg=f"sample {b} {r}")


def test_equals_the_two_step_device_path(yv):
    """yv_train_crops == yv_augment_patchify on the host-transformed crop; layout 0 == yv_crop_resize_norm(layout=0)."""
    from utils.trainClass import _EvalTransform
    from yvhip.augment import identity_record
    S, P = 224, 16
    imgs, pool, table = _pool(SIZES, seed=3)
    plan = np.array(_rects(S), dtype=np.int32)
    geo, idx = _records(S, len(plan), seed=4)
    t = _EvalTransform((S, S))
    x = np.stack([np.transpose(t(image=imgs[r[0]][r[2]:r[4], r[1]:r[3]])["image"], (2, 0, 1)) for r in plan])
    dgeo, didx = torch.from_numpy(geo).to(DEV), torch.from_numpy(idx).to(DEV)
    two_step = yv.augment_patchify(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), dgeo, didx, P)
    dpool, dtable, dplan = (torch.from_numpy(a).to(DEV) for a in (pool, table, plan))
    assert torch.equal(yv.train_crops(dpool, dtable, dplan, dgeo, didx, S, P), two_step)
    # same-size images: the only case the inference kernel accepts
    same, spool, stable = _pool([(320, 200)] * 3, seed=8)
    rects = [(0, 0, 0, 320, 200), (1, 7, 9, 300, 60), (2, 100, 100, 101, 180), (2, 0, 199, 320, 200), (1, 250, 20, 320, 190)]
    crop_list = torch.tensor([list(r) + [0] for r in rects], dtype=torch.int32, device=DEV)
    old = yv.crop_resize_norm(torch.from_numpy(np.stack(same)).to(DEV), crop_list, None, len(rects), S, P, layout=0)
    gi, ii = identity_record(S)
    new = yv.train_crops(torch.from_numpy(spool).to(DEV), torch.from_numpy(stable).to(DEV),
                         torch.tensor(rects, dtype=torch.int32, device=DEV), torch.from_numpy(np.stack([gi] * len(rects))).to(DEV),
                         torch.from_numpy(np.stack([ii] * len(rects))).to(DEV), S, P, layout=0)
    assert new.dtype == torch.float32 and torch.equal(new, old)


def test_hostile_records_stay_in_bounds(yv):
    """Ids, rectangles, tables and matrices come from the host and the image table from a buffer the caller filled: all are
    clamped as include/yv_hip.h states, never trusted.  The numpy statement applies the same clamps."""
    from yvhip.augment import identity_record
    S, P = 64, 8
    _, pool, table = _pool([(50, 40), (9, 200), (120, 3)], seed=0)
    table = np.concatenate([table, [[pool.size + 10 ** 9, 77, 77], [-5, 0, -3], [0, 10 ** 9, 10 ** 9]]]).astype(np.int64)   # lying rows
    plans = [(-7, 0, 0, 50, 40), (99, 0, 0, 9, 200), (0, -30, -30, 90, 90), (1, 5, 5, 5, 5), (2, 100, 2, 20, 1),
             (0, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1), (1, 10 ** 6, 10 ** 6, 10 ** 6 + 3, 10 ** 6 + 3), (2, 0, 0, 120, 3),
             (3, 0, 0, 77, 77), (4, 0, 0, 10, 10), (5, 0, 0, 50, 40), (0, 10, 10, 40, 30)]
    B = len(plans)
    recs = [identity_record(S) for _ in range(B)]
    recs[0][0][0:6] = (np.nan, 1e30, -1e30, np.inf, 0.0, np.nan)
    recs[1][1][36:] = np.random.default_rng(1).integers(-10 ** 6, 10 ** 6, 2 * S)
    recs[2][1][0:4] = (7, -3, 2, 1000)
    recs[2][1][4:36] = np.random.default_rng(2).integers(-500, 500, 32)
    recs[3][0][6:] = np.random.default_rng(3).uniform(-1e6, 1e6, 2 * S)
    recs[6][1][36:] = np.random.default_rng(4).integers(-2 ** 31, 2 ** 31 - 1, 2 * S)
    recs[11][0][0:6] = (1e30, 0, 0, 0, np.nan, 0)
    geo, idx = np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs])
    plan = np.array(plans, dtype=np.int32)
    got = _run(yv, pool, table, plan, geo, idx, S, P)                      # returning at all means YV_OK (check() raises otherwise)
    np.testing.assert_array_equal(got, em.train_crops_reference(pool, table, plan, geo, idx, S, P, 2))
    gi, ii = np.stack([identity_record(S)[0]] * B), np.stack([identity_record(S)[1]] * B)
    got0 = _run(yv, pool, table, plan, gi, ii, S, 0, layout=0)
    np.testing.assert_array_equal(got0, em.train_crops_reference(pool, table, plan, gi, ii, S, 0, 0))


def test_argument_checks(yv):
    S = 64
    pool = torch.zeros(300, dtype=torch.uint8, device=DEV)
    table = torch.tensor([[0, 10, 10]], dtype=torch.int64, device=DEV)
    plan = torch.tensor([[0, 0, 0, 10, 10]], dtype=torch.int32, device=DEV)
    geo = torch.zeros(1, 6 + 2 * S, device=DEV)
    idx = torch.zeros(1, 36 + 2 * S, dtype=torch.int32, device=DEV)
    assert tuple(yv.train_crops(pool, table, plan, geo, idx, S, 16).shape) == (16, 768)
    bad = [
        (pool.float(), table, plan, geo, idx, S, 16),                       # wrong dtypes
        (pool, table.int(), plan, geo, idx, S, 16),
        (pool, table, plan.long(), geo, idx, S, 16),
        (pool, table, plan, geo.double(), idx, S, 16),
        (pool, table, plan, geo, idx.long(), S, 16),
        (pool, table, plan, geo[:, :-1].contiguous(), idx, S, 16),         # wrong record widths
        (pool, table, plan, geo, idx[:, :-2].contiguous(), S, 16),
        (pool, table, plan[:, :4].contiguous(), geo, idx, S, 16),
        (pool, table[:, :2].contiguous(), plan, geo, idx, S, 16),
        (pool.cpu(), table, plan, geo, idx, S, 16),                         # host tensors
        (pool, table, plan.cpu(), geo, idx, S, 16),
        (pool, table, plan, geo, idx, S, 12),                               # patch must be a multiple of 8 dividing S
        (pool[:2].contiguous(), table, plan, geo, idx, S, 16),
    ]
    for args in bad:
        with pytest.raises(yv.YvError):
            yv.train_crops(*args)
    with pytest.raises(yv.YvError):
        yv.train_crops(pool, table, plan, geo, idx, S, 16, layout=1)
    assert yv.lib.yv_train_crops(None, 300, None, 1, None, 1, S, 16, None, None, 2, None, None) == -1


# ------------------------------------------------------------------------------------------------- end to end
def _epoch(tc, yv, wpath, objs, circ, vobjs, vcirc, seed, device_pool, bs):
    """One train_one_epoch + valid_one_epoch over fresh loaders and a fresh net; records every step's operand and loss."""
    tc.set_seed(seed)
    tf = tc.build_transforms(tc.CFG)
    kw = {"device_pool": True} if device_pool else {}
    train_loader, valid_loader = tc.build_dataloader(objs, circ, vobjs, vcirc, tf, **kw)
    net = tc.build_model(tc.CFG, pretrained=wpath, modelName="vit_tiny_test").to(DEV)
    tr = tc._trainer_for(net, None)
    ops, losses, real = [], [], tr.step

    def spy(patches, labels, lr):
        loss, logits = real(patches, labels, lr)
        ops.append((patches.clone(), labels.clone()))
        losses.append(loss.clone())
        return loss, logits

    tr.step = spy
    correct = tc.train_one_epoch(net, None, train_loader, tc.build_loss, None, [0.01], bs, 0, 2, True, DEV)
    acc, vloss = tc.valid_one_epoch(net, tc.build_loss, valid_loader)
    torch.cuda.synchronize()
    return dict(ops=ops, losses=torch.cat(losses).cpu(), sd={k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                correct=correct, val=(acc, vloss), loader=train_loader)


def test_epoch_equals_host_loader_epoch(yv, tmp_path, monkeypatch):
    """Control first: two host-loader epochs after the same set_seed.  Then host against device loader: the patch operand and
    the labels of every step are identical; where the control showed bit-identical losses and weights (this trainer has no
    atomics on its path, so it normally does), the loss sequence, the final state dict and the validation results are too -
    otherwise only the operands are gated, and the assertion message of the control says so."""
    import utils.trainClass as tc
    from yvhip import engines
    from yvhip.crop_loader import CropBatch, DeviceCropLoader
    bs = 6
    monkeypatch.setattr(tc.CFG, "train_bs", bs, raising=False)
    monkeypatch.setattr(tc.CFG, "valid_bs", 4, raising=False)
    random.seed(0)
    objs, circ = tc.xml2pd([em.write_dataset(tmp_path / "tr", seed=1, n_images=7)])
    vobjs, vcirc = tc.xml2pd([em.write_dataset(tmp_path / "va", seed=2, n_images=4, many=3)])
    n = len(objs) + len(circ)
    assert n % bs != 0                                               # the short-batch skip is exercised
    wpath = str(tmp_path / "w.pth")
    torch.save(engines.init_vit_wrapper_state("vit_tiny_test", tc.CFG.num_classes, seed=8), wpath)
    h1, h2, d = (_epoch(tc, yv, wpath, objs, circ, vobjs, vcirc, 5, dp, bs) for dp in (False, False, True))
    assert isinstance(d["loader"], DeviceCropLoader) and isinstance(next(iter(d["loader"]))[0], CropBatch)
    assert len(h1["ops"]) == len(h2["ops"]) == len(d["ops"]) == n // bs
    for (p1, l1), (p2, l2) in zip(h1["ops"], h2["ops"]):
        assert torch.equal(p1, p2) and torch.equal(l1, l2), "control: the host loader itself is not repeatable"
    for k, ((p1, l1), (p2, l2)) in enumerate(zip(h1["ops"], d["ops"])):
        assert p1.dtype == p2.dtype == torch.bfloat16 and torch.equal(p1.view(torch.int16), p2.view(torch.int16)), f"step {k}"
        assert torch.equal(l1, l2), f"step {k}"
    control_exact = torch.equal(h1["losses"], h2["losses"]) and all(torch.equal(h1["sd"][k], h2["sd"][k]) for k in h1["sd"])
    print(f"control: host epochs bit-identical in loss and weights: {control_exact}")
    if control_exact:
        assert torch.equal(h1["losses"], d["losses"])
        assert all(torch.equal(h1["sd"][k], d["sd"][k]) for k in h1["sd"])
        assert h1["correct"] == d["correct"] and h1["val"] == d["val"]


@pytest.mark.parametrize("train_dtype", [None, "mxfp8"])
def test_train_with_device_loader_from_xml_directories(yv, tmp_path, monkeypatch, train_dtype):
    """utils.trainClass.train(CFG) with CFG.device_loader = True: pool from the xml directories, epochs of the native step,
    best.pth + result.json (mirror of test_train_class_from_xml_directories)."""
    import utils.trainClass as tc
    from yvhip import crop_loader
    monkeypatch.setattr(tc.CFG, "train_bs", 2, raising=False)
    monkeypatch.setattr(tc.CFG, "valid_bs", 4, raising=False)
    em.write_dataset(tmp_path / "tr", seed=1, n_images=6, many=4)
    em.write_dataset(tmp_path / "va", seed=2, n_images=3, many=2)
    launches, decodes = [], []
    real, real_dec = yv.train_crops, crop_loader._decode
    monkeypatch.setattr(yv, "train_crops", lambda *a, **k: (launches.append(a[7] if len(a) > 7 else k.get("layout", 2)), real(*a, **k))[1])
    monkeypatch.setattr(crop_loader, "_decode", lambda p: (decodes.append(p), real_dec(p))[1])

    class C(tc.CFG):
        modelName = "vit_tiny_test"
        pretrained = str(tmp_path / "missing.pth")
        train_path = [str(tmp_path / "tr"), str(tmp_path / "does_not_exist")]
        valid_path = [str(tmp_path / "va")]
        epoch, lr = 2, 5e-3
        img_size = [224, 224]
        device_loader = True
    if train_dtype:
        C.train_dtype = train_dtype
    random.seed(1)
    res = tc.train(C, log=str(tmp_path / "result.json"), save_path=str(tmp_path / "out" / "best.pth"))
    assert sorted(res) == [1, 2] and all(0.0 <= r["val_acc"] <= 100.0 and np.isfinite(r["loss"]) for r in res.values())
    assert sorted(json.load(open(tmp_path / "result.json"))) == ["1", "2"]
    assert len(decodes) == len(set(decodes)) == 9                    # every image decoded once for both epochs
    assert launches.count(2) > 0 and launches.count(0) > 0           # training operands and validation batches
    if any(r["val_acc"] > 0 for r in res.values()):
        sd = torch.load(tmp_path / "out" / "best.pth", map_location="cpu", weights_only=True)
        assert "model.cls_token" in sd and "fc.3.weight" in sd
    assert os.path.exists(tmp_path / "result.json")
