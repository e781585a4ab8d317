"""Device-resident crop loader for classifier fine-tuning (opt-in: `utils.trainClass.build_dataloader(device_pool=True)`,
`CFG.device_loader`).

The host loader (utils/trainClass.py:227-273) decodes the source image of EVERY annotated object on every visit, resizes
and normalises the crop in numpy and ships it as f32 CHW (600 KB at 224 x 224).  Here every distinct source image is decoded
once into one flat u8 buffer on the device (`DevicePool`); a batch is then only a PLAN - image id and crop rectangle per
sample - and `yv_train_crops` (csrc/train_crops.hip) gathers, resizes, normalises, augments and patchifies it in one pass.

RNG-order contract: the plan dataset is iterated by a torch `DataLoader` with the host loader's batch size / shuffle /
drop_last, and its `__getitem__` draws from Python's `random` exactly what `build_dataset.__getitem__` + `crop_image` draw
(one `random.random()` for the circle switch, then the four `randint` of the training inflate).  After the same `set_seed`
both loaders therefore visit the same objects with the same rectangles, and `train_one_epoch` draws the same augmentation
records, so the patch operands are byte-identical.
"""
from __future__ import annotations

import random
from typing import Callable, Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import YvError
from .augment import identity_record

DEFAULT_POOL_BYTES = 32 << 30          # of the MI355X's 288 GB: leaves the trainer, its workspaces and the allocator ample room


def _image_size(path: str) -> Tuple[int, int]:
    """(width, height) from the file header; nothing is decoded."""
    with Image.open(path) as im:
        return im.size


def _decode(path: str) -> np.ndarray:
    """(H, W, 3) u8, the call of crop_image (utils/trainClass.py:72)."""
    return np.asarray(Image.open(path).convert('RGB'))


class DevicePool:
    """Every distinct image of `paths`, decoded once, RGB, row-major, tightly packed in one flat u8 buffer, plus the table
    {byte offset, width, height} (i64) `yv_train_crops` reads.  `device=None` keeps both as host arrays (no GPU needed);
    otherwise they are uploaded as `pool` / `table` tensors.  Raises YvError when the images need more than `max_bytes`."""

    def __init__(self, paths: Iterable[str], device=None, max_bytes: int = DEFAULT_POOL_BYTES):
        self.paths: List[str] = list(dict.fromkeys(paths))
        if not self.paths:
            raise YvError("DevicePool: no images")
        self.index: Dict[str, int] = {p: i for i, p in enumerate(self.paths)}
        self.sizes: List[Tuple[int, int]] = [_image_size(p) for p in self.paths]          # (width, height) per image, host side
        nbytes = [3 * w * h for w, h in self.sizes]
        self.nbytes = int(sum(nbytes))
        if self.nbytes > max_bytes:
            raise YvError(f"DevicePool: {len(self.paths)} decoded images need {self.nbytes} bytes, the pool cap is {max_bytes} "
                          "bytes (raise max_bytes or train with the host loader)")
        table = np.zeros((len(self.paths), 3), dtype=np.int64)
        table[:, 0] = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
        table[:, 1:] = self.sizes
        buf = np.empty(self.nbytes, dtype=np.uint8)
        for p, (off, w, h) in zip(self.paths, table.tolist()):
            a = _decode(p)
            if a.shape != (h, w, 3):
                raise YvError(f"DevicePool: {p} decoded to {a.shape}, its header says {(h, w, 3)}")
            buf[off:off + 3 * w * h] = a.reshape(-1)
        self.host_pool, self.host_table = buf, table
        self.device = None if device is None else torch.device(device)
        self.pool = self.table = None
        if self.device is not None:
            self.pool = torch.from_numpy(buf).to(self.device)
            self.table = torch.from_numpy(table).to(self.device)
            self.host_pool = None                                    # the device copy is the pool; keep no second one
        self._identity = {}

    def __len__(self):
        return len(self.paths)

    def image_id(self, path: str) -> int:
        try:
            return self.index[path]
        except KeyError:
            raise YvError(f"DevicePool: {path} is not in the pool") from None

    def image(self, i: int) -> np.ndarray:
        """(H, W, 3) u8 view of image i in the host buffer (pools built with device=None)."""
        if self.host_pool is None:
            raise YvError("DevicePool.image: the pool lives on the device")
        off, w, h = self.host_table[i].tolist()
        return self.host_pool[off:off + 3 * w * h].reshape(h, w, 3)

    def identity_records(self, B: int, S: int):
        key = (B, S)
        if key not in self._identity:
            g, i = identity_record(S)
            self._identity[key] = (np.stack([g] * B), np.stack([i] * B))
        return self._identity[key]


class CropBatch:
    """What the device loader yields in place of a (B,3,S,S) tensor: the plan (B,5) i32 {image id, x0, y0, x1, y1}."""

    def __init__(self, pool: DevicePool, plan: np.ndarray, size: int):
        self.pool, self.plan, self.size = pool, np.ascontiguousarray(plan, dtype=np.int32), int(size)

    @property
    def shape(self):
        return (self.plan.shape[0], 3, self.size, self.size)

    def _launch(self, geo: np.ndarray, idx: np.ndarray, patch: int, layout: int) -> torch.Tensor:
        from . import train_crops
        pool = self.pool
        if pool.device is None:
            raise YvError("CropBatch: the pool was built with device=None; there is no CPU path for the crop kernel")
        B, S = self.plan.shape[0], self.size
        geo = np.ascontiguousarray(geo, dtype=np.float32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if geo.shape != (B, 6 + 2 * S) or idx.shape != (B, 36 + 2 * S):
            raise YvError(f"CropBatch: records of shape {geo.shape} / {idx.shape} do not fit {B} samples of size {S}")
        # one H2D copy for the whole batch: records and plan are all 4-byte words
        flat = np.concatenate([geo.view(np.int32).reshape(-1), idx.reshape(-1), self.plan.reshape(-1)])
        d = torch.from_numpy(flat).to(pool.device)
        ng, ni = geo.size, idx.size
        return train_crops(pool.pool, pool.table, d[ng + ni:].view(B, 5), d[:ng].view(torch.float32).view(B, 6 + 2 * S),
                           d[ng:ng + ni].view(B, 36 + 2 * S), S, patch, layout)

    def patch_operand(self, geo: np.ndarray, idx: np.ndarray, patch: int) -> torch.Tensor:
        """(B*(S/P)^2, 3*P*P) bf16 rows: crops with the augmentation records applied (one yv_train_crops launch)."""
        return self._launch(geo, idx, patch, 2)

    def images(self) -> torch.Tensor:
        """(B,3,S,S) f32 normalised crops, no augmentation (validation)."""
        return self._launch(*self.pool.identity_records(self.plan.shape[0], self.size), 0, 0)


class PlanDataset(torch.utils.data.Dataset):
    """build_dataset (utils/trainClass.py:227-273) with the pixels left out: items are (plan row, one-hot int64, path).  Draws
    from `random` what the host dataset draws, in its order; width / height come from the pool instead of an opened file."""

    def __init__(self, pool: DevicePool, objects: Sequence[dict], objects_circle: Sequence[dict], val: bool,
                 inflate: Callable, num_classes: int, transforms=None):
        self.pool, self.objects, self.objects_circle, self.val = pool, objects, objects_circle, val
        self.inflate, self.num_classes, self.transforms = inflate, num_classes, transforms
        self.lenth_cir, self.lenth = len(objects_circle), len(objects)
        self.rate = self.lenth_cir / (self.lenth + self.lenth_cir) if (self.lenth + self.lenth_cir) > 0 else 0
        if val:
            self.dataset = list(objects) + list(objects_circle)

    def __len__(self):
        return len(self.objects_circle) + len(self.objects)

    def __getitem__(self, index):
        if not self.val:
            if random.random() > self.rate:
                obj = self.objects[index % self.lenth if self.lenth > 0 else 0]
            else:
                obj = self.objects_circle[index % self.lenth_cir if self.lenth_cir > 0 else 0]
        else:
            obj = self.dataset[index]
        o = obj['objects']
        img = self.pool.image_id(obj["path"])
        w, h = self.pool.sizes[img]
        x0, y0, x1, y1 = self.inflate(o["xmin"], o["ymin"], o["xmax"], o["ymax"], w, h, not self.val)
        if x1 <= x0 or y1 <= y0:
            raise YvError(f"degenerate crop ({x0}, {y0}, {x1}, {y1}) for box ({o['xmin']}, {o['ymin']}, {o['xmax']}, {o['ymax']}) "
                          f"in {obj['path']} ({w} x {h})")
        plan = torch.tensor([img, x0, y0, x1, y1], dtype=torch.int32)
        label = torch.nn.functional.one_hot(torch.tensor(o["label"]), num_classes=self.num_classes)
        return plan, label.to(torch.int64), obj["path"]


class DeviceCropLoader:
    """Iterates like the host loaders and yields (batch, one-hot targets, paths).  Training form (`training=True`, shuffled):
    batch is a `CropBatch`; `train_one_epoch` asks it for the patch operand.  Validation form (in order, eval inflate): batch is
    the (B,3,S,S) f32 device tensor `valid_one_epoch` / `Network_Wrapper.forward` take - or the `CropBatch` itself when the
    pool was built with device=None."""

    def __init__(self, pool: DevicePool, objects, objects_circle, batch_size: int, size: int, inflate: Callable,
                 num_classes: int, training: bool, transforms=None):
        from torch.utils.data import DataLoader
        self.pool, self.size, self.training, self.batch_size = pool, int(size), training, batch_size
        self.dataset = PlanDataset(pool, objects, objects_circle, not training, inflate, num_classes, transforms)
        self.loader = DataLoader(self.dataset, batch_size=batch_size, num_workers=0, shuffle=training, drop_last=False)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for plan, targets, paths in self.loader:
            batch = CropBatch(self.pool, plan.numpy(), self.size)
            if not self.training and self.pool.device is not None:
                batch = batch.images()
            yield batch, targets, paths
