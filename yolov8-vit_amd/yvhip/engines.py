"""Host-side execution plans for the two networks of the hot path.

`YoloEngine`  - YOLOv8 (n/s/m) backbone + neck + Detect head + DFL decode
`VitEngine`   - timm-layout ViT (patch 16) + Network_Wrapper head (rows B3, B4)

Both consume state dicts in the key layout of the packages the reference uses
(`ultralytics` fused model: `model.{i}...conv.weight/bias`; `Network_Wrapper(timm ViT)`:
`model.*` + `fc.1.*`/`fc.3.*`, utils/utils.py:59-87) and replay a fixed list of C-ABI
launches on the current stream.  No tensor math happens in PyTorch: torch only owns the
device buffers.  Activations are NHWC bf16; concat / split / upsample never materialise
(operand views + dual-source gather in the conv kernel).
"""
from __future__ import annotations

import functools
import math
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from .extent import n_anchors, net_hw
from .guard import StepGuard
from . import (CONV_DMA32_64, CONV_DMA32_96, CONV_DMA32_128, EPI_GELU, EPI_OUT_F32, EPI_POSEMB, EPI_RES_BF16, EPI_RES_F32, EPI_SILU,
               RES_LN_WIDTHS, YvError, attention, attention_cls, attention_fp8, attention_long, attention_mxfp8, c2f_fused, cls_rows, conv2d,
               conv2d_group, conv2d_instance, conv2d_mxfp8, detect_decode,
               detect_tail, get_option, layernorm, layernorm_mxfp8, linear, linear_ln, linear_mxfp8, linear_mxfp8_q, linear_res_ln, mx_map,
               mx_view, quant_conv_weight_mxfp8, quant_mxfp8, quant_mxfp8_map, require_gpu, set_option, sppf_pool, stem_conv,
               view, wrapper_head)

# --------------------------------------------------------------------------------------- YOLOv8
YOLO_SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768)}
REG_MAX = 16
LAYER_STRIDE = {0: 2, 1: 4, 2: 4, 3: 8, 4: 8, 5: 16, 6: 16, 7: 32, 8: 32, 9: 32, 12: 16, 15: 8, 16: 16, 18: 16,
                19: 32, 21: 32}


def _c(ch: int, scale: str) -> int:
    _, w, mx = YOLO_SCALES[scale]
    return int(math.ceil(min(ch, mx) * w / 8) * 8)


def _n(rep: int, scale: str) -> int:
    return max(round(rep * YOLO_SCALES[scale][0]), 1)


def yolo_layers(scale: str):
    """(index, kind, params) of yolov8.yaml at this scale; `src` = skip connection layer."""
    c = lambda v: _c(v, scale)
    n = lambda v: _n(v, scale)
    return [
        (0, "stem", dict(cout=c(64))),
        (1, "conv", dict(cin=c(64), cout=c(128))),
        (2, "c2f", dict(cin=c(128), cout=c(128), n=n(3), add=True)),
        (3, "conv", dict(cin=c(128), cout=c(256))),
        (4, "c2f", dict(cin=c(256), cout=c(256), n=n(6), add=True)),
        (5, "conv", dict(cin=c(256), cout=c(512))),
        (6, "c2f", dict(cin=c(512), cout=c(512), n=n(6), add=True)),
        (7, "conv", dict(cin=c(512), cout=c(1024))),
        (8, "c2f", dict(cin=c(1024), cout=c(1024), n=n(3), add=True)),
        (9, "sppf", dict(cin=c(1024), cout=c(1024))),
        (12, "c2f", dict(cin=c(1024) + c(512), cout=c(512), n=n(3), add=False, a=(9, 1), b=(6, 0))),
        (15, "c2f", dict(cin=c(512) + c(256), cout=c(256), n=n(3), add=False, a=(12, 1), b=(4, 0))),
        (16, "conv", dict(cin=c(256), cout=c(256))),
        (18, "c2f", dict(cin=c(256) + c(512), cout=c(512), n=n(3), add=False, a=(16, 0), b=(12, 0))),
        (19, "conv", dict(cin=c(512), cout=c(512))),
        (21, "c2f", dict(cin=c(512) + c(1024), cout=c(1024), n=n(3), add=False, a=(19, 0), b=(9, 0))),
    ]


def detect_widths(scale: str, nc: int) -> Tuple[Tuple[int, int, int], int, int, int]:
    """Detect head: (input channels per scale, width of the box branch, width of the class branch, nc padded to a multiple of 8)."""
    ch = (_c(256, scale), _c(512, scale), _c(1024, scale))
    return ch, max(16, ch[0] // 4, REG_MAX * 4), max(ch[0], min(nc, 100)), (nc + 7) // 8 * 8


def yolo_conv_keys(scale: str, nc: int) -> List[Tuple[str, int, int, int]]:
    """(state-dict prefix, cin, cout, k) of every conv in the fused model."""
    out = []
    for idx, kind, p in yolo_layers(scale):
        pre = f"model.{idx}."
        if kind == "stem":
            out.append((pre + "conv", 3, p["cout"], 3))
        elif kind == "conv":
            out.append((pre + "conv", p["cin"], p["cout"], 3))
        elif kind == "c2f":
            c = p["cout"] // 2
            out.append((pre + "cv1.conv", p["cin"], 2 * c, 1))
            out.append((pre + "cv2.conv", (2 + p["n"]) * c, p["cout"], 1))
            for j in range(p["n"]):
                out.append((pre + f"m.{j}.cv1.conv", c, c, 3))
                out.append((pre + f"m.{j}.cv2.conv", c, c, 3))
        elif kind == "sppf":
            out.append((pre + "cv1.conv", p["cin"], p["cin"] // 2, 1))
            out.append((pre + "cv2.conv", p["cin"] * 2, p["cout"], 1))
    ch, c2, c3, _ = detect_widths(scale, nc)
    for s, ci in enumerate(ch):
        out += [(f"model.22.cv2.{s}.0.conv", ci, c2, 3), (f"model.22.cv2.{s}.1.conv", c2, c2, 3),
                (f"model.22.cv2.{s}.2", c2, 4 * REG_MAX, 1), (f"model.22.cv3.{s}.0.conv", ci, c3, 3),
                (f"model.22.cv3.{s}.1.conv", c3, c3, 3), (f"model.22.cv3.{s}.2", c3, nc, 1)]
    return out


def init_yolo_state(scale: str = "n", nc: int = 5, seed: int = 42, head_gain: float = 1.0,
                    cls_bias: float = 0.0) -> Dict[str, torch.Tensor]:
    """Seeded random fused weights (BN folded to identity) in the ultralytics key layout.
    There is no network on the box: checkpoints cannot be fetched, so benchmarks and
    smoke tests use this.  `head_gain` widens the spread of the Detect outputs."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for key, ci, co, k in yolo_conv_keys(scale, nc):
        gain = head_gain if key.endswith(".2") else 1.0
        sd[key + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (gain * math.sqrt(2.0 / (ci * k * k)))
        sd[key + ".bias"] = torch.randn(co, generator=g) * 0.1
        if key.startswith("model.22.cv3.") and key.endswith(".2"):
            sd[key + ".bias"] += cls_bias
    sd["model.22.dfl.conv.weight"] = torch.arange(REG_MAX, dtype=torch.float32).view(1, REG_MAX, 1, 1)
    return sd


def _fused_c2f_block(p: dict) -> bool:
    """The C2f blocks YoloEngine runs as one yv_c2f_fused launch (c <= 32)."""
    c = p["cout"] // 2
    return "a" not in p and p["add"] and p["cin"] == p["cout"] and c in (16, 32) and p["n"] in (1, 2)


# ---- the detector's launch list: entries of four kinds.  Buffers go by name: out{idx} (a layer's output), y{idx} (the concat
# buffer of a C2f / SPPF block), t{idx} (a bottleneck's hidden map), det{s}.hb / .hc (the head's feature maps), det{s}.box / .cls
class Stem(NamedTuple):
    key: str
    out: str


class Conv(NamedTuple):
    key: str                    # of the weight and bias tables (a state-dict prefix, det{s}.0 or a padded 1 x 1 of the head)
    srcs: tuple                 # one or two (buffer, channel offset, channels, up): the input views, concatenated
    k: int
    stride: int
    out: str
    out_off: int                # channel offset in `out`
    res_off: Optional[int]      # channel offset in `out` of the bf16 residual, None = no residual
    flags: int                  # epilogue
    cout: int
    down: int                   # the output grid is (H // down) x (W // down)
    block: Optional[int]        # index of the C2f block the convolution is part of


class C2fFused(NamedTuple):
    src: str
    out: str
    c: int
    n: int
    cv1: str
    m: tuple                    # keys of m.0.cv1, m.0.cv2, m.1.cv1, ...
    cv2: str


class Pool(NamedTuple):
    buf: str                    # SPPF: three chained 5 x 5 max-pools of channels [0, c) into the three chunks behind them
    c: int


class ConvGroup(NamedTuple):
    convs: tuple                # Conv entries that are independent of each other: one conv2d_group call (grouped_head)


@functools.lru_cache(maxsize=None)
def detect_launches(scale: str, nc: int = 5, fused_c2f: bool = True, tail: bool = True, grouped_head: bool = False) -> tuple:
    """What YoloEngine launches in front of the decode, in order: Stem, Conv, C2fFused and Pool entries.  fused_c2f: the blocks of
    _fused_c2f_block as one entry each, else layer by layer.  tail=False: without the last 1 x 1 convolutions of the head (the
    fused Detect tail runs them).  grouped_head: the head's convolutions as ConvGroup entries, one per step - the three det{s}.0,
    the six .1, (tail) the six .2 - behind the unchanged backbone and neck."""
    layers = yolo_layers(scale)
    width = {idx: p["cout"] for idx, _, p in layers}
    out: list = []

    def conv(key, srcs, k, stride, obuf, cout, down, out_off=0, res_off=None, flags=EPI_SILU, block=None):
        flags |= EPI_RES_BF16 if res_off is not None else 0
        out.append(Conv(key, tuple(srcs), k, stride, obuf, out_off, res_off, flags, cout, down, block))

    for idx, kind, p in layers:
        pre, d, o = f"model.{idx}.", LAYER_STRIDE[idx], f"out{idx}"
        src = [(f"out{idx - 1}", 0, p.get("cin"), 0)]
        if kind == "stem":
            out.append(Stem(pre + "conv", o))
        elif kind == "conv":
            conv(pre + "conv", src, 3, 2, o, p["cout"], d)
        elif kind == "c2f":
            c, n, y, t = p["cout"] // 2, p["n"], f"y{idx}", f"t{idx}"
            m = [pre + f"m.{j}.cv{i}.conv" for j in range(n) for i in (1, 2)]
            if fused_c2f and _fused_c2f_block(p):       # one launch, intermediates in LDS (YOLOv8n: model.2, model.4)
                out.append(C2fFused(src[0][0], o, c, n, pre + "cv1.conv", tuple(m), pre + "cv2.conv"))
                continue
            if "a" in p:                                # the neck: concat of two layers' outputs, one of them upsampled
                src = [(f"out{i}", 0, width[i], up) for i, up in (p["a"], p["b"])]
            conv(pre + "cv1.conv", src, 1, 1, y, 2 * c, d, block=idx)
            for j in range(n):
                at = (1 + j) * c
                conv(m[2 * j], [(y, at, c, 0)], 3, 1, t, c, d, block=idx)
                conv(m[2 * j + 1], [(t, 0, c, 0)], 3, 1, y, c, d, at + c, at if p["add"] else None, block=idx)
            conv(pre + "cv2.conv", [(y, 0, (2 + n) * c, 0)], 1, 1, o, p["cout"], d, block=idx)
        elif kind == "sppf":
            c_, y = p["cin"] // 2, f"y{idx}"
            conv(pre + "cv1.conv", src, 1, 1, y, c_, d)
            out.append(Pool(y, c_))
            conv(pre + "cv2.conv", [(y, 0, 4 * c_, 0)], 1, 1, o, p["cout"], d)
    ch, c2, c3, ncp = detect_widths(scale, nc)
    for s, fidx in enumerate((15, 18, 21)):
        d, hb, hc = LAYER_STRIDE[fidx], f"det{s}.hb", f"det{s}.hc"
        conv(f"det{s}.0", [(f"out{fidx}", 0, ch[s], 0)], 3, 1, hb, c2 + c3, d)
        conv(f"model.22.cv2.{s}.1.conv", [(hb, 0, c2, 0)], 3, 1, hc, c2, d)
        conv(f"model.22.cv3.{s}.1.conv", [(hb, c2, c3, 0)], 3, 1, hc, c3, d, c2)
        if tail:
            conv(f"model.22.cv2.{s}.2", [(hc, 0, c2, 0)], 1, 1, f"det{s}.box", 4 * REG_MAX, d, flags=EPI_OUT_F32)
            conv(f"model.22.cv3.{s}.2.pad", [(hc, c2, c3, 0)], 1, 1, f"det{s}.cls", ncp, d, flags=EPI_OUT_F32)
    if grouped_head:                # per level the head is 1 + 2 (+ 2) entries, step after step; the levels do not meet
        per = 5 if tail else 3
        head, out = out[-3 * per:], out[:-3 * per]
        for step in ((0,), (1, 2), (3, 4))[:2 + tail]:
            out.append(ConvGroup(tuple(head[s * per + i] for s in range(3) for i in step)))
    return tuple(out)


# layer kinds (kernel size, stride, whether Cin % 128 == 0) whose MXFP8 launches measured slower than the bf16 ones on the
# MI355X (tools/conv_mx_bench.py under rocprofv3, YOLOv8m at 64 images, profiles/conv_mx_layers.txt):
# the 1 x 1 layers, +19 % / +21 %.  They stay bf16.
MX_SLOW_KINDS: Tuple[Tuple[int, int, bool], ...] = ((1, 1, False), (1, 1, True))
# narrowest layers kept in bf16 for accuracy: a convolution reading or writing fewer than 96 channels stays bf16.  Measured
# (tools/mx_plan_accuracy.py): with every eligible layer YOLOv8n's smallest per-anchor cosine against the bf16 engine is 0.975,
# with this floor 0.996 (s 0.992, m 0.994) - the floor of 0.99 holds for every scale.
MX_MIN_WIDTH = 96


def mx_conv_plan(scale: str, nc: int = 5, speed_filter: bool = True, min_width: Optional[int] = None) -> List[str]:
    """Convolutions YoloEngine(dtype="mxfp8") runs on the block-scaled MXFP8 kernel (yv_conv2d_mxfp8), in execution order.
    A convolution qualifies when every channel count and channel offset it reads (input views, concat sources) and its
    output channels are multiples of 32 (one E8M0 scale per 32 channels of a pixel).  Stays bf16: the stem (3 input
    channels), model.1 of scales whose stem writes 48 / 16 / 32 channels below that, whole C2f blocks whose hidden width
    c is not a multiple of 32 (their bottleneck chunks straddle scale blocks; YOLOv8m model.2, c = 48), the fused C2f
    blocks (one yv_c2f_fused launch), SPPF's cv2 (reads the bf16 max-pool chunks) and the last 1 x 1 convolutions of the
    head (read by yv_detect_tail / the decode); then the layer kinds of MX_SLOW_KINDS (speed_filter) and the layers
    narrower than MX_MIN_WIDTH channels (min_width overrides it)."""
    launches = detect_launches(scale, nc)
    pooled = {e.buf for e in launches if isinstance(e, Pool)}
    a32 = lambda e: all(x % 32 == 0 for x in (e.cout, e.out_off, *(x for _, off, c, _ in e.srcs for x in (off, c))))
    convs = [e for e in launches if isinstance(e, Conv) and not e.flags & EPI_OUT_F32 and e.srcs[0][0] not in pooled]
    straddling = {e.block for e in convs if e.block is not None and not a32(e)}
    mw = MX_MIN_WIDTH if min_width is None else min_width
    out: List[str] = []
    for e in convs:
        widths = [c for _, _, c, _ in e.srcs]
        if not a32(e) or e.block in straddling:
            continue
        if speed_filter and (e.k, e.stride, sum(widths) % 128 == 0) in MX_SLOW_KINDS:
            continue
        if min(*widths, e.cout) < mw:
            continue
        out.append(e.key)
    return out


def dma32_layers(scale: str, nc: int, B: int, hw) -> List[str]:
    """Keys of the Conv entries of detect_launches(scale, nc) that YoloEngine at B images of hw = (H, W) pixels launches on
    cgemm_dma32_kernel under the CURRENT options (host only: conv2d_instance of each entry's shape, output and residual stride;
    empty while "conv_dma32" is 0).  An MXFP8 engine runs those of them that are not in mx_conv_plan."""
    ld = {}
    for idx, kind, p in yolo_layers(scale):
        ld[f"out{idx}"] = p["cout"]
        if kind == "c2f":
            ld[f"y{idx}"], ld[f"t{idx}"] = (2 + p["n"]) * (p["cout"] // 2), p["cout"] // 2
        elif kind == "sppf":
            ld[f"y{idx}"] = p["cin"] * 2
    _, c2, c3, ncp = detect_widths(scale, nc)
    for s in range(3):
        ld.update({f"det{s}.hb": c2 + c3, f"det{s}.hc": c2 + c3, f"det{s}.box": 4 * REG_MAX, f"det{s}.cls": ncp})
    H, W = hw
    out = []
    for e in detect_launches(scale, nc):
        if type(e) is not Conv:
            continue
        c = [x[2] for x in e.srcs] + [0]
        code = conv2d_instance(B, H // e.down, W // e.down, e.k, e.stride, c[0], c[1], e.cout, ld[e.out],
                               ld[e.out] if e.res_off is not None else 0, e.flags)
        if code & 15 in (CONV_DMA32_64, CONV_DMA32_96, CONV_DMA32_128):
            out.append(e.key)
    return out


SMALL_MAP_PIXELS = 12800   # "conv_small" of a YoloEngine(small_maps=True) pass: the bound measured in DESIGN.md section 32


def _env_flag(value: Optional[bool], var: str) -> bool:
    """An opt-in constructor flag: the argument where one is given, else the environment variable `var` ("1" = on, unset = off)."""
    return os.environ.get(var, "0") == "1" if value is None else bool(value)


def _khwc(w: torch.Tensor) -> torch.Tensor:
    """(Cout,Cin,k,k) f32 -> (Cout, k*k*Cin) bf16 with K order (ky,kx,cin)."""
    co = w.shape[0]
    return w.permute(0, 2, 3, 1).reshape(co, -1).contiguous().to(torch.bfloat16)


class YoloEngine:
    """images (B,H,W,3) u8 RGB on the device -> boxes (B,A,4) f32 xyxy, scores (B,A,nc) f32."""

    def __init__(self, state: Dict[str, torch.Tensor], scale: str = "n", nc: int = 5, size=640,
                 device: str = "cuda:0", dtype: str = "bf16", small_maps: Optional[bool] = None,
                 grouped_head: Optional[bool] = None, dma32: Optional[bool] = None):
        """size: the network input's side, or its (H, W); both sides multiples of 32.  `hw` is always (H, W); `size` is the int
        of a square engine and the pair of a rectangular one.  The launch list does not depend on the extent.
        dtype "bf16" (default) or "mxfp8": the convolutions of mx_conv_plan(scale, nc) then run on OCP e4m3 operands with
        one E8M0 scale per 32 input channels (yv_conv2d_mxfp8; weights quantised once here), their inputs kept as MX maps
        next to the bf16 activations; the rest of the network is unchanged.
        small_maps (opt-in, both dtypes): the pass runs with the option "conv_small" at SMALL_MAP_PIXELS, so its bf16 convolutions
        with 64-aligned channels on maps of at most that many output pixels - the lower levels at the one or few images a request
        carries - take cgemm_small_kernel's 64- / 32-pixel tiles; the option is restored afterwards.  None:
        the environment variable YV_YOLO_SMALL_MAPS ("1" = on, unset = off).  Off: the option is not touched.  The launch list
        and the MXFP8 convolutions are the same either way.
        grouped_head (opt-in, both dtypes): each step of the Detect head - the three det{s}.0, the six .1, the six .2 where the
        tail is not fused - is one conv2d_group call: the levels' convolutions on the same kernel instance share one grid (DESIGN.md
        section 33).  The MXFP8 convolutions of an mxfp8 engine and the members conv2d_group does not group run alone; every
        output keeps its bits.  None: the environment variable YV_YOLO_GROUPED_HEAD ("1" = on, unset = off).  Composes with
        small_maps: the group is routed inside the same "conv_small" window.
        dma32 (opt-in, both dtypes): the pass runs with the option "conv_dma32" at 1, so its bf16 convolutions whose input channels
        are a multiple of 32 but not of 64 (dma32_layers: YOLOv8m's 96- and 288-channel layers) take cgemm_dma32_kernel instead of
        igemm_kernel; the option is restored afterwards.  None: the environment variable YV_YOLO_DMA32
        ("1" = on, unset = off).  Off: the option is not touched.  The launch list and the MXFP8 convolutions are the same either
        way; the eligibility is disjoint from that of small_maps and grouped_head, so the flags compose."""
        require_gpu()
        hw = net_hw(size)
        if dtype not in ("bf16", "mxfp8"):
            raise YvError("dtype must be 'bf16' or 'mxfp8'")
        self.dtype = dtype
        self.small_maps = _env_flag(small_maps, "YV_YOLO_SMALL_MAPS")
        self.grouped_head = _env_flag(grouped_head, "YV_YOLO_GROUPED_HEAD")
        self.dma32 = _env_flag(dma32, "YV_YOLO_DMA32")
        self.scale, self.nc, self.dev = scale, nc, torch.device(device)
        self.layers = yolo_layers(scale)
        self.w: Dict[str, torch.Tensor] = {}
        self.b: Dict[str, torch.Tensor] = {}
        need = yolo_conv_keys(scale, nc)
        for key, ci, co, k in need:
            wt, bs = state[key + ".weight"], state[key + ".bias"]
            if tuple(wt.shape) != (co, ci, k, k):
                raise YvError(f"{key}.weight has shape {tuple(wt.shape)}, expected {(co, ci, k, k)}")
            if key == "model.0.conv":
                self.w[key] = wt.float().permute(2, 3, 1, 0).reshape(27, co).contiguous().to(self.dev)    # (tap*3+c, cout)
            else:
                self.w[key] = _khwc(wt.float()).to(self.dev)
            self.b[key] = bs.float().contiguous().to(self.dev)
        _, self.c2, self.c3, self.ncp = detect_widths(scale, nc)
        for s in range(3):
            # horizontal fusion of the two 3x3 convs that share the scale's feature map (test.ipynb:1285)
            k0, k1 = f"model.22.cv2.{s}.0.conv", f"model.22.cv3.{s}.0.conv"
            self.w[f"det{s}.0"] = torch.cat([self.w[k0], self.w[k1]], 0).contiguous()
            self.b[f"det{s}.0"] = torch.cat([self.b[k0], self.b[k1]], 0).contiguous()
            kc = f"model.22.cv3.{s}.2"                       # class logits: pad Cout to a multiple of 8
            wp = torch.zeros(self.ncp, self.c3, dtype=torch.bfloat16, device=self.dev)
            wp[:nc] = self.w[kc]
            bp = torch.zeros(self.ncp, dtype=torch.float32, device=self.dev)
            bp[:nc] = self.b[kc]
            self.w[kc + ".pad"], self.b[kc + ".pad"] = wp, bp
            wp16 = torch.zeros(16, self.c3, dtype=torch.bfloat16, device=self.dev)     # operand of the fused tail: one MFMA row fragment
            bp16 = torch.zeros(16, dtype=torch.float32, device=self.dev)
            if nc <= 16:
                wp16[:nc] = self.w[kc]
                bp16[:nc] = self.b[kc]
            self.w[kc + ".pad16"], self.b[kc + ".pad16"] = wp16, bp16
        # fused Detect tail (yv_detect_tail: last 1 x 1 convolutions + DFL decode + sigmoid in one launch, bit-identical)
        self.fused_tail = self.c2 == 64 and nc <= 16 and self.c3 in (64, 128, 192)
        self.fused_c2f = True                    # backbone C2f blocks with c <= 32 in one launch each (yv_c2f_fused)
        self.mx_layers: List[str] = mx_conv_plan(scale, nc) if dtype == "mxfp8" else []
        # (e4m3 (Cout, Kpad), K-step-major scales) of the MX convolutions
        self.wq: Dict[str, tuple] = {key: quant_conv_weight_mxfp8(self.w[key]) for key in self.mx_layers}
        if self.wq:
            torch.cuda.synchronize(self.dev)
        heads = [(f"model.22.cv2.{s}.2", f"model.22.cv3.{s}.2.pad16") for s in range(3)]
        self._tail_operands = ([self.w[k] for k, _ in heads], [self.b[k] for k, _ in heads],
                               [self.w[k] for _, k in heads], [self.b[k] for _, k in heads])
        self._set_extent(hw)

    def _set_extent(self, hw: Tuple[int, int]):
        """What depends on the input extent: the sizes, the anchor count, the buffer sets and their guard."""
        self.hw = hw
        self.size = hw[0] if hw[0] == hw[1] else hw
        self.A = n_anchors(*hw)
        self._bufs: Dict[int, dict] = {}
        self.guard = StepGuard()                 # one replay of the launch list at a time (callers may be threads)

    def resized(self, size) -> "YoloEngine":
        """A sibling engine for another input extent (an int or (H, W)): it shares this engine's weight, bias, MX weight and
        tail-operand tensors (nothing is uploaded or quantised again) and has buffers and a StepGuard of its own.  It keeps the
        small_maps, grouped_head and dma32 flags."""
        hw = net_hw(size)
        sib = object.__new__(type(self))
        sib.__dict__.update(self.__dict__)
        sib._set_extent(hw)
        return sib

    # -- buffers are allocated once per batch size and reused (no allocation in the step)
    def _buffers(self, B: int) -> dict:
        """"flat": the launch list's buffers by name; "out": the layers' outputs by index; "mx": the MX maps by buffer name."""
        if B in self._bufs:
            return self._bufs[B]
        H, W = self.hw
        bf = lambda d, c: torch.zeros((B, H // d, W // d, c), dtype=torch.bfloat16, device=self.dev)
        f32 = lambda d, c: torch.zeros((B, H // d, W // d, c), dtype=torch.float32, device=self.dev)
        flat: Dict[str, torch.Tensor] = {}
        for idx, kind, p in self.layers:
            d = LAYER_STRIDE[idx]
            flat[f"out{idx}"] = bf(d, p["cout"])
            if kind == "c2f":
                c = p["cout"] // 2
                flat[f"y{idx}"] = bf(d, (2 + p["n"]) * c)
                flat[f"t{idx}"] = bf(d, c)
            elif kind == "sppf":
                flat[f"y{idx}"] = bf(d, p["cin"] * 2)
        for s, d in enumerate((8, 16, 32)):
            flat[f"det{s}.hb"] = bf(d, self.c2 + self.c3)
            flat[f"det{s}.hc"] = bf(d, self.c2 + self.c3)
            flat[f"det{s}.box"] = f32(d, 4 * REG_MAX)
            flat[f"det{s}.cls"] = f32(d, self.ncp)
        # every bf16 activation an MX convolution reads gets an MX map next to it, written by its producers (bf16 engine: none)
        mx_convs = [e for e in detect_launches(self.scale, self.nc) if type(e) is Conv and e.key in self.wq]
        read = sorted({b for e in mx_convs for b, *_ in e.srcs})
        bufs = self._bufs[B] = dict(
            flat=flat, out={idx: flat[f"out{idx}"] for idx, _, _ in self.layers},
            mx={n: mx_map(B, flat[n].shape[1], flat[n].shape[2], flat[n].shape[3], self.dev) for n in read},
            **{x: [flat[f"det{s}.{x}"] for s in range(3)] for x in ("hc", "box", "cls")})
        return bufs

    def _produced(self, bufs, name: str, c_off: int, c: int):
        """A bf16 producer wrote channels [c_off, c_off+c) of `name`: bring its MX map, if it has one, up to date."""
        if name in bufs["mx"]:
            quant_mxfp8_map(bufs["flat"][name], bufs["mx"][name], c_off, c, c_off)

    def _conv_group(self, bufs, B: int, e: ConvGroup):
        """One step of the head: the MXFP8 members alone, the bf16 members as one conv2d_group call, then their MX maps."""
        flat = bufs["flat"]
        members, bf16 = [], [c for c in e.convs if c.key not in self.wq]
        for c in e.convs:
            if c.key in self.wq:
                self._conv(bufs, B, c)
        for c in bf16:
            v = [view(flat[b], off, ch, up) for b, off, ch, up in c.srcs]
            out = flat[c.out]
            members.append((v[0], v[1] if len(v) > 1 else None, B, self.hw[0] // c.down, self.hw[1] // c.down, c.k, c.stride,
                            self.w[c.key], self.b[c.key], out, c.out_off, c.flags, out if c.res_off is not None else None,
                            c.res_off or 0))
        if members:
            conv2d_group(members)
        for c in bf16:
            self._produced(bufs, c.out, c.out_off, c.cout)

    def _conv(self, bufs, B: int, e: Conv):
        flat, mx = bufs["flat"], bufs["mx"]
        h, wd, out = self.hw[0] // e.down, self.hw[1] // e.down, flat[e.out]
        res = out if e.res_off is not None else None
        if e.key in self.wq:
            wq, ws = self.wq[e.key]
            v = [mx_view(mx[b], off, c, up) for b, off, c, up in e.srcs]
            conv2d_mxfp8(v[0], v[1] if len(v) > 1 else None, B, h, wd, e.k, e.stride, wq, ws, self.b[e.key], out, e.out_off,
                         e.flags, res=res, res_c_off=e.res_off or 0, out_mx=mx.get(e.out), outq_c_off=e.out_off)
        else:
            v = [view(flat[b], off, c, up) for b, off, c, up in e.srcs]
            conv2d(v[0], v[1] if len(v) > 1 else None, B, h, wd, e.k, e.stride, self.w[e.key], self.b[e.key], out, e.out_off,
                   e.flags, res=res, res_c_off=e.res_off or 0)
            self._produced(bufs, e.out, e.out_off, e.cout)

    def forward_raw(self, images: torch.Tensor):
        """Runs backbone+neck+head; returns per-scale (box logits f32, class logits f32) NHWC tensors.  Called with `self.guard`
        held (as __call__ does) the engine-owned buffers themselves are returned - valid until the caller leaves the guard;
        called bare, the result is CLONED under the guard, so that another thread's next replay cannot overwrite what this
        caller is still reading."""
        outer = self.guard.held
        with self.guard:
            res = self._forward_raw(images)
            if outer:
                return res
            return tuple([t.clone() for t in part] for part in res)

    def _forward_raw(self, images: torch.Tensor, tail: bool = True):
        want = {}                               # the options of this pass (small_maps, dma32): set around it, restored after it
        if self.small_maps:
            want["conv_small"] = SMALL_MAP_PIXELS
        if self.dma32:
            want["conv_dma32"] = 1
        if not want:
            return self._launch_list(images, tail)
        saved = {k: get_option(k) for k in want}
        for k, v in want.items():
            set_option(k, v)
        try:
            return self._launch_list(images, tail)
        finally:
            for k, v in saved.items():
                set_option(k, v)

    def _launch_list(self, images: torch.Tensor, tail: bool = True):
        """Walks detect_launches (self.fused_c2f is read here, so it may be flipped between calls).  tail=False: stop in front of
        the last 1 x 1 convolutions and return the per-scale feature buffers (B,Hs,Ws,c2+c3)."""
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise YvError("images must be (B,H,W,3) uint8")
        B = images.shape[0]
        if tuple(images.shape[1:3]) != self.hw:
            raise YvError(f"engine built for {self.hw[0]}x{self.hw[1]}")
        bufs = self._buffers(B)
        flat, w, b = bufs["flat"], self.w, self.b
        for e in detect_launches(self.scale, self.nc, bool(self.fused_c2f), tail, bool(self.grouped_head)):
            if type(e) is Conv:
                self._conv(bufs, B, e)
            elif type(e) is ConvGroup:
                self._conv_group(bufs, B, e)
            elif type(e) is Pool:
                sppf_pool(flat[e.buf], e.c)
            else:
                if type(e) is Stem:
                    stem_conv(images, w[e.key], b[e.key], flat[e.out])
                else:
                    c2f_fused(flat[e.src], e.c, e.n, w[e.cv1], b[e.cv1], [w[k] for k in e.m], [b[k] for k in e.m], w[e.cv2],
                              b[e.cv2], flat[e.out])
                self._produced(bufs, e.out, 0, flat[e.out].shape[-1])
        return (list(bufs["box"]), list(bufs["cls"])) if tail else (list(bufs["hc"]), [])

    def __call__(self, images: torch.Tensor):
        with self.guard:                         # the decode reads the engine-owned head buffers
            if self.fused_tail:
                feats, _ = self._forward_raw(images, tail=False)
                return detect_tail(feats, self.c3, *self._tail_operands, self.size, self.nc)
            box_l, cls_l = self._forward_raw(images)
            return detect_decode(box_l, cls_l, self.size, self.nc)


# ------------------------------------------------------------------------------------------ ViT
VIT_CFGS = {
    "vit_base_patch16_224": (16, 768, 12, 12),
    "vit_base_patch8_224": (8, 768, 12, 12),            # the reference's configured model (utils/class_config.py:21)
    "vit_large_patch16_224": (16, 1024, 24, 16),        # BASELINE.json configs[4]
    "vit_tiny_test": (16, 128, 2, 2),
    "vit_tiny8_test": (8, 128, 2, 2),
}


MID_GEMM_ROWS = 3152      # "linear_mid" of a VitEngine(mid_gemm=True) pass: the bound measured in DESIGN.md section 31
MX_MID_GEMM_ROWS = 3152   # "linear_mx_mid" of a VitEngine(dtype="mxfp8", mid_gemm=True) pass: DESIGN.md section 38


def vit_cfg(name: str):
    base = name.split(".")[0]
    if base not in VIT_CFGS:
        raise YvError(f"classifier '{name}' is not supported by the MI355X path (supported: {sorted(VIT_CFGS)})")
    return VIT_CFGS[base]


def init_vit_wrapper_state(name: str, num_classes: int = 5, seed: int = 42, img: int = 224) -> Dict[str, torch.Tensor]:
    """Seeded random Network_Wrapper(timm ViT) state dict (`model.*` + `fc.1.*`, `fc.3.*`)."""
    P, D, L, H = vit_cfg(name)
    n = (img // P) ** 2 + 1
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=0.02: torch.randn(*s, generator=g) * scale
    sd = {"model.cls_token": rn(1, 1, D), "model.pos_embed": rn(1, n, D),
          "model.patch_embed.proj.weight": rn(D, 3, P, P), "model.patch_embed.proj.bias": rn(D)}
    for i in range(L):
        p = f"model.blocks.{i}."
        sd[p + "norm1.weight"] = 1 + rn(D); sd[p + "norm1.bias"] = rn(D)
        sd[p + "attn.qkv.weight"] = rn(3 * D, D, scale=0.04); sd[p + "attn.qkv.bias"] = rn(3 * D)
        sd[p + "attn.proj.weight"] = rn(D, D); sd[p + "attn.proj.bias"] = rn(D)
        sd[p + "norm2.weight"] = 1 + rn(D); sd[p + "norm2.bias"] = rn(D)
        sd[p + "mlp.fc1.weight"] = rn(4 * D, D); sd[p + "mlp.fc1.bias"] = rn(4 * D)
        sd[p + "mlp.fc2.weight"] = rn(D, 4 * D); sd[p + "mlp.fc2.bias"] = rn(D)
    sd["model.norm.weight"] = 1 + rn(D); sd["model.norm.bias"] = rn(D)
    sd["model.head.weight"] = rn(1000, D, scale=0.05); sd["model.head.bias"] = rn(1000, scale=0.5)
    sd["fc.1.weight"] = rn(128, 1000, scale=0.05); sd["fc.1.bias"] = rn(128, scale=0.1)
    sd["fc.3.weight"] = rn(num_classes, 128, scale=0.2); sd["fc.3.bias"] = rn(num_classes, scale=0.1)
    return sd


class VitEngine:
    """Patch-major bf16 crops (cap*tok, 3*P*P) -> backbone logits (cap, 1024-padded) f32 and,
    through the Network_Wrapper head, class logits (cap, nc) + labels (cap)."""

    long_attn = False                                   # opt-in (see __init__)
    ln_gemm = False
    fp8_attn = False

    def __init__(self, state: Dict[str, torch.Tensor], name: str, num_classes: int = 5, img: int = 224,
                 device: str = "cuda:0", dtype: str = "bf16", cls_tail: bool = True, fused_ln: Optional[bool] = None,
                 long_attn: Optional[bool] = None, mid_gemm: Optional[bool] = None, ln_gemm: Optional[bool] = None,
                 fp8_attn: Optional[bool] = None):
        """cls_tail (bf16 path): the last block runs on the cls rows only - nothing reads its other rows (see _last_block_cls);
        False gives the full last block.  The mxfp8 pass runs every block in full whatever cls_tail says, and it ignores
        full_cus_from (the attribute PipelinedRunner sets): both are properties of the bf16 block loop.
        dtype "bf16" (default) or "mxfp8": the four block linears (qkv, proj, fc1, fc2) then run on OCP e4m3 operands
        with one E8M0 scale per 32 K elements through the block-scaled MFMA (BASELINE.json configs[4]); weights are
        quantised once here, activations by yv_quant_mxfp8 in front of each GEMM; everything else (patch-embed, LayerNorm,
        attention, residual stream, heads) keeps its bf16 / f32 form.
        fused_ln (bf16 path, opt-in): proj and fc2 run as linear_res_ln, which also writes the LayerNorm their result feeds (the
        block's norm2 / the next block's norm1), so the separate LayerNorm passes over the residual stream go away - see
        _blocks_bf16.  None reads the environment variable YV_VIT_FUSED_LN ("1" = on, unset = off; a bf16 engine only, the
        mxfp8 engine ignores the variable).  True with dtype "mxfp8" or an embedding width yv_linear_res_ln lacks: YvError.
        long_attn (both dtypes, opt-in): the full blocks' attention runs as attention_long (128-row query blocks, pipelined 64-key
        tiles; dtype "mxfp8": writing the proj operand directly) in place of attention / attention_mxfp8.  Effective only where the
        engine's token count exceeds 224 (/8 models at 224, /16 models at 384): a shorter-sequence engine accepts the flag and
        keeps calling attention, whose single-tile kernel is the tuned one there.  attention_cls of the cls tail is unchanged.
        None reads the environment variable YV_VIT_LONG_ATTN ("1" = on, unset = off).  Works together with fused_ln and cls_tail.
        mid_gemm (opt-in): the pass runs with the option "linear_mid" at MID_GEMM_ROWS, so its bf16 linears of 257 .. that many
        rows - the block products at a handful of crops, as DetectClassifyPipeline(fit_crops=True) sizes them - take
        gemm_mid_kernel's 64 x 64 tiles instead of 128 x 128 ones; the option is restored after the pass.  None reads the
        environment variable YV_VIT_MID_GEMM ("1" = on, unset = off).  Off: the option is not touched.  dtype "mxfp8": the pass
        also runs with "linear_mx_mid" at MX_MID_GEMM_ROWS (restored after it), so its four block linears - linear_mxfp8 and the
        fc1 -> fc2 hand-over linear_mxfp8_q - take gemm_mx_mid_kernel's 64 x 64 tiles wherever "linear_mx_mid_fill" admits the shape,
        from one crop on.  This is the one combination whose results differ from mid_gemm=False in the last bits (another order
        of the K sum); an mxfp8 engine without the flag never touches the option.
        ln_gemm (bf16 path, opt-in): norm1 -> qkv and norm2 -> fc1 of the full blocks run as linear_ln, and the pass runs with the
        option "linear_ln_mid" at MID_GEMM_ROWS (restored after it): at 257 .. that many rows, where "linear_ln_fill" admits the
        shape, each pair is ONE launch whose 64 x 64 tiles normalise their own rows; at any other size - one crop of a /16 model,
        a batch - linear_ln runs the layernorm + linear pair as before.  The cls tail, the final LayerNorm and the mxfp8 pass are
        unchanged.  None reads the environment variable YV_VIT_LN_GEMM ("1" = on, unset = off; a bf16 engine without fused_ln
        only, any other ignores the variable).  True with fused_ln or dtype "mxfp8": YvError.  Independent of mid_gemm, long_attn
        and cls_tail.
        fp8_attn (mxfp8 path, opt-in): the qkv product of every block is linear_mxfp8_q(flags=0) into the MXFP8 buffer pair
        qkv8 / qkv8s (the bf16 qkv buffer is not allocated) and the attention is attention_fp8 - QK^T on the block-scaled FP8 MFMA,
        V dequantised in the kernel, the proj operand written directly - whatever the token count; it takes precedence over
        long_attn and YV_MX_ATTN_FUSED.  Q, K and V are then rounded to e4m3: the results differ from the unflagged engine's
        (DESIGN.md section 40).  None reads the environment variable YV_VIT_FP8_ATTN ("1" = on, unset = off; an mxfp8 engine only,
        a bf16 engine ignores the variable).  True with dtype "bf16": YvError.  Works together with mid_gemm."""
        require_gpu()
        if dtype not in ("bf16", "mxfp8"):
            raise YvError("dtype must be 'bf16' or 'mxfp8'")
        self.dtype = dtype
        self.cls_tail = bool(cls_tail)
        self.fused_ln = _env_flag(fused_ln, "YV_VIT_FUSED_LN") and (fused_ln is not None or dtype == "bf16")
        if self.fused_ln and dtype != "bf16":
            raise YvError("fused_ln is a property of the bf16 path (dtype='mxfp8' hands LayerNorm outputs over in MXFP8)")
        self.long_attn = _env_flag(long_attn, "YV_VIT_LONG_ATTN")
        self.mid_gemm = _env_flag(mid_gemm, "YV_VIT_MID_GEMM")
        self.ln_gemm = _env_flag(ln_gemm, "YV_VIT_LN_GEMM") and (ln_gemm is not None or (dtype == "bf16" and not self.fused_ln))
        if self.ln_gemm and (dtype != "bf16" or self.fused_ln):
            raise YvError("ln_gemm is a property of the bf16 path without fused_ln (which leaves no LayerNorm in front of a linear)")
        self.fp8_attn = _env_flag(fp8_attn, "YV_VIT_FP8_ATTN") and (fp8_attn is not None or dtype == "mxfp8")
        if self.fp8_attn and dtype != "mxfp8":
            raise YvError("fp8_attn is a property of the mxfp8 path (the bf16 engine has no MXFP8 qkv operand)")
        self.fuse_attention_quant = os.environ.get("YV_MX_ATTN_FUSED", "1") == "1"     # A/B switch of the mxfp8 path
        self.P, self.D, self.L, self.H = vit_cfg(name)
        if self.D // self.H != 64:
            raise YvError("attention kernel is specialised for head dim 64")
        if self.fused_ln and self.D not in RES_LN_WIDTHS:
            raise YvError(f"fused_ln: yv_linear_res_ln has no instance for width {self.D} (has {RES_LN_WIDTHS})")
        self.name, self.nc, self.img, self.dev = name, num_classes, img, torch.device(device)
        self.tok = (img // self.P) ** 2
        self.N = self.tok + 1
        dev, D = self.dev, self.D
        bf = lambda t: t.float().contiguous().to(torch.bfloat16).to(dev)
        f32 = lambda t: t.float().contiguous().to(dev)
        g = lambda k: state["model." + k]
        self.w_pe = bf(g("patch_embed.proj.weight").reshape(D, -1))
        self.b_pe = f32(g("patch_embed.proj.bias"))
        self.cls = f32(g("cls_token").reshape(D))
        self.pos = f32(g("pos_embed").reshape(self.N, D))
        self.blocks = []
        for i in range(self.L):
            p = f"blocks.{i}."
            self.blocks.append(dict(
                n1w=f32(g(p + "norm1.weight")), n1b=f32(g(p + "norm1.bias")),
                wqkv=bf(g(p + "attn.qkv.weight")), bqkv=f32(g(p + "attn.qkv.bias")),
                wproj=bf(g(p + "attn.proj.weight")), bproj=f32(g(p + "attn.proj.bias")),
                n2w=f32(g(p + "norm2.weight")), n2b=f32(g(p + "norm2.bias")),
                wfc1=bf(g(p + "mlp.fc1.weight")), bfc1=f32(g(p + "mlp.fc1.bias")),
                wfc2=bf(g(p + "mlp.fc2.weight")), bfc2=f32(g(p + "mlp.fc2.bias"))))
        if dtype == "bf16":                              # last block, cls tail: the query and the K | V parts of the qkv product
            last = self.blocks[-1]
            last["wq"], last["bq"], last["wkv"], last["bkv"] = last["wqkv"][:D], last["bqkv"][:D], last["wqkv"][D:], last["bqkv"][D:]
        if dtype == "mxfp8":
            if D % 128:
                raise YvError("mxfp8 needs an embedding width that is a multiple of 128")
            for blk in self.blocks:
                for k in ("wqkv", "wproj", "wfc1", "wfc2"):
                    blk[k + "_q"], blk[k + "_s"] = quant_mxfp8(blk[k])
                    del blk[k]
        self.nw, self.nb = f32(g("norm.weight")), f32(g("norm.bias"))
        wh = torch.zeros(1024, D)
        wh[:1000] = g("head.weight").float()
        bh = torch.zeros(1024)
        bh[:1000] = g("head.bias").float()
        self.w_head, self.b_head = bf(wh), f32(bh)
        self.fc1w, self.fc1b = f32(state["fc.1.weight"].float().t()), f32(state["fc.1.bias"])     # (1000,128): transposed
        self.fc2w, self.fc2b = f32(state["fc.3.weight"]), f32(state["fc.3.bias"])
        if tuple(self.fc2w.shape) != (num_classes, 128):
            raise YvError("fc.3.weight does not match num_classes")
        self._bufs: Dict[tuple, dict] = {}
        self._guards: Dict[int, StepGuard] = {}
        # PipelinedRunner: first block whose persistent GEMMs take every CU again (the reduced budget exists for the detector of the
        # NEXT batch, which runs beside the first part of a classifier pass only); None = one budget for the whole pass
        self.full_cus_from: Optional[int] = None

    def guard(self, slot: int = 0) -> StepGuard:
        """Guard of one buffer set: hold it across backbone() + head() (the features live in engine-owned buffers).
        Different slots are independent (the split classifier runs two of them concurrently on two streams)."""
        g = self._guards.get(slot)
        if g is None:
            g = self._guards.setdefault(slot, StepGuard())
        return g

    def _buffers(self, cap: int, slot: int = 0) -> dict:
        """Activation buffers for `cap` crops; `slot` selects an independent set (concurrent sub-batches)."""
        key = (cap, slot)
        if key not in self._bufs:
            dev, D, N = self.dev, self.D, self.N
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            rp = (cap * N + 255) // 256 * 256
            # fp8_attn: the qkv product is an MXFP8 operand image (bytes + K-step-major block scales) instead of the bf16 buffer
            qkv = dict(qkv=z((cap * N, 3 * D), torch.bfloat16)) if not self.fp8_attn else \
                dict(qkv8=z((cap * N, 3 * D), torch.uint8), qkv8s=z((3 * D // 128, rp, 4), torch.uint8))
            self._bufs[key] = dict(
                x=z((cap * N, D), torch.float32), h=z((cap * N, D), torch.bfloat16),
                **qkv, o=z((cap * N, D), torch.bfloat16),
                g=z((cap * N, 4 * D), torch.bfloat16), c=z((cap, D), torch.bfloat16),
                # compact cls-row operands of the pruned last block: q, attention output, LN2 output, GELU output
                tq=z((cap, D), torch.bfloat16), to=z((cap, D), torch.bfloat16), th=z((cap, D), torch.bfloat16),
                tg=z((cap, 4 * D), torch.bfloat16),
                **({} if self.dtype != "mxfp8" else dict(          # MXFP8 operand images: bytes + K-step-major block scales
                    q=z((cap * N, D), torch.uint8), qs=z((D // 128, (cap * N + 255) // 256 * 256, 4), torch.uint8),
                    gq=z((cap * N, 4 * D), torch.uint8),
                    gs=z((4 * D // 128, (cap * N + 255) // 256 * 256, 4), torch.uint8))),
                feats=z((cap, 1024), torch.float32))
        return self._bufs[key]

    def patch_buffer(self, cap: int, slot: int = 0) -> torch.Tensor:
        b = self._buffers(cap, slot)
        if "pm" not in b:
            b["pm"] = torch.zeros((cap * self.tok, 3 * self.P * self.P), dtype=torch.bfloat16, device=self.dev)
        return b["pm"]

    def backbone(self, patches: torch.Tensor, cap: int, count: Optional[torch.Tensor] = None, slot: int = 0) -> torch.Tensor:
        """patches (cap*tok, 3*P*P) bf16 -> feats (cap,1024) f32 (columns >= 1000 are zero padding)."""
        outer = self.guard(slot).held
        with self.guard(slot):
            feats = self._backbone(patches, cap, count, slot)
            return feats if outer else feats.clone()         # bare call: a copy that the next replay cannot overwrite

    def _backbone(self, patches: torch.Tensor, cap: int, count: Optional[torch.Tensor], slot: int) -> torch.Tensor:
        if not self.ln_gemm:
            return self._backbone_mid(patches, cap, count, slot)
        ln_mid = get_option("linear_ln_mid")
        set_option("linear_ln_mid", MID_GEMM_ROWS)
        try:
            return self._backbone_mid(patches, cap, count, slot)
        finally:
            set_option("linear_ln_mid", ln_mid)

    def _backbone_mid(self, patches: torch.Tensor, cap: int, count: Optional[torch.Tensor], slot: int) -> torch.Tensor:
        if not self.mid_gemm:
            return self._backbone_tail(patches, cap, count, slot)
        mid = get_option("linear_mid")
        mx_mid = get_option("linear_mx_mid") if self.dtype == "mxfp8" else None
        set_option("linear_mid", MID_GEMM_ROWS)
        if mx_mid is not None:
            set_option("linear_mx_mid", MX_MID_GEMM_ROWS)
        try:
            return self._backbone_tail(patches, cap, count, slot)
        finally:
            set_option("linear_mid", mid)
            if mx_mid is not None:
                set_option("linear_mx_mid", mx_mid)

    def _backbone_tail(self, patches: torch.Tensor, cap: int, count: Optional[torch.Tensor], slot: int) -> torch.Tensor:
        if self.cls_tail:
            return self._backbone_pass(patches, cap, count, slot)
        skinny = get_option("linear_skinny")            # the full path as it was before the cls tail: its kernels, its bits
        set_option("linear_skinny", 0)
        try:
            return self._backbone_pass(patches, cap, count, slot)
        finally:
            set_option("linear_skinny", skinny)

    def _backbone_pass(self, patches: torch.Tensor, cap: int, count: Optional[torch.Tensor], slot: int) -> torch.Tensor:
        b = self._buffers(cap, slot)
        D, N, tok = self.D, self.N, self.tok
        x = b["x"]
        cls_rows(self.cls, self.pos, cap, tok, D, x)
        linear(patches, self.w_pe, self.b_pe, x, flags=EPI_OUT_F32 | EPI_POSEMB, pos=self.pos, tok=tok, m_dev=count,
               m_mul=tok)
        (self._blocks_mxfp8 if self.dtype == "mxfp8" else self._blocks_bf16)(b, cap, count)
        layernorm(x, self.nw, self.nb, b["c"], cap, D, N * D, D, count_dev=count, rows_per_count=1)
        linear(b["c"], self.w_head, self.b_head, b["feats"], flags=EPI_OUT_F32, m_dev=count, m_mul=1)
        return b["feats"]

    def _attention(self, b: dict, cap: int, count: Optional[torch.Tensor], mx: bool = False):
        """Attention of a full block, qkv -> o: attention_long where the flag is on and the sequence long enough, else attention.
        mx: the result is the proj operand (q, qs) instead - written by the kernel itself (attention_long, or attention_mxfp8 unless
        YV_MX_ATTN_FUSED=0), else by a quantisation pass over o.  Both MX kernels take an even head count, which an mxfp8 engine
        always has: H = D / 64 and D is a multiple of 128."""
        N, H = self.N, self.H
        if self.fp8_attn:                                # an mxfp8 engine: the qkv operand is MXFP8 (see _blocks_mxfp8), any N
            attention_fp8(b["qkv8"], b["qkv8s"], cap, N, H, r_dev=count, out_q=b["q"], out_scale=b["qs"])
            return
        qkv, o = b["qkv"], b["o"]
        long = self.long_attn and N > 224
        if mx and long:
            attention_long(qkv, cap, N, H, r_dev=count, out_q=b["q"], out_scale=b["qs"])
        elif mx and self.fuse_attention_quant:
            attention_mxfp8(qkv, cap, N, H, b["q"], b["qs"], r_dev=count)
        else:
            (attention_long if long else attention)(qkv, cap, N, H, o, r_dev=count)
            if mx:
                quant_mxfp8(o, b["q"], b["qs"])

    def _blocks_bf16(self, b: dict, cap: int, count: Optional[torch.Tensor]):
        D, N = self.D, self.N
        x, h, qkv, o, gbuf = b["x"], b["h"], b["qkv"], b["o"], b["g"]
        rows = cap * N
        # fused_ln: every proj also writes its block's norm2 output and every fc2 (but the last block's) the NEXT block's norm1 output
        # (linear_res_ln), so of the 2L block LayerNorms only block 0's norm1 - its input comes from patch-embed + cls_rows - remains
        # ln_gemm: norm1 -> qkv and norm2 -> fc1 are linear_ln calls (one launch where its route fuses, else the same pair; h is
        # written on the pair route only - nothing else reads it in a full block)
        fused, ln_gemm = self.fused_ln, self.ln_gemm
        for i, blk in enumerate(self.blocks):
            if self.full_cus_from is not None and i == self.full_cus_from:
                set_option("linear_p8_cus", 0)          # the caller (PipelinedRunner) restores its own setting after the pass
            if self.cls_tail and i == self.L - 1:
                self._last_block_cls(b, blk, cap, count, norm1_done=fused and i > 0)
                break
            if ln_gemm:
                linear_ln(x, blk["n1w"], blk["n1b"], h, blk["wqkv"], blk["bqkv"], qkv, m_dev=count, m_mul=N)
            else:
                if not (fused and i > 0):
                    layernorm(x, blk["n1w"], blk["n1b"], h, rows, D, D, D, count_dev=count, rows_per_count=N)
                linear(h, blk["wqkv"], blk["bqkv"], qkv, m_dev=count, m_mul=N)
            self._attention(b, cap, count)
            if fused:
                linear_res_ln(o, blk["wproj"], blk["bproj"], x, blk["n2w"], blk["n2b"], h, m_dev=count, m_mul=N)
            else:
                linear(o, blk["wproj"], blk["bproj"], x, flags=EPI_RES_F32, m_dev=count, m_mul=N)
                if not ln_gemm:
                    layernorm(x, blk["n2w"], blk["n2b"], h, rows, D, D, D, count_dev=count, rows_per_count=N)
            if ln_gemm:
                linear_ln(x, blk["n2w"], blk["n2b"], h, blk["wfc1"], blk["bfc1"], gbuf, flags=EPI_GELU, m_dev=count, m_mul=N)
            else:
                linear(h, blk["wfc1"], blk["bfc1"], gbuf, flags=EPI_GELU, m_dev=count, m_mul=N)
            if fused and i + 1 < self.L:
                nxt = self.blocks[i + 1]
                linear_res_ln(gbuf, blk["wfc2"], blk["bfc2"], x, nxt["n1w"], nxt["n1b"], h, m_dev=count, m_mul=N)
            else:
                linear(gbuf, blk["wfc2"], blk["bfc2"], x, flags=EPI_RES_F32, m_dev=count, m_mul=N)

    def _last_block_cls(self, b: dict, blk: dict, cap: int, count: Optional[torch.Tensor], norm1_done: bool = False):
        """The last block on the cls rows.  The final LayerNorm and the head read row 0 of each crop only, and inside a block token
        rows meet only in attention, through K and V: so K | V are computed for every row, and the query, the attention, proj, LN2,
        fc1 and fc2 for the `cap` cls rows.  Only the cls rows of x are updated; the operands in between are compact (cap, *).
        norm1_done (fused_ln): the previous block's fc2 launch already wrote this block's norm1 output into h."""
        D, N, H = self.D, self.N, self.H
        x, h, qkv = b["x"], b["h"], b["qkv"]
        if "xc" not in b:                                                   # views, made once per buffer set
            b["xc"], b["hc"], b["kv"] = x[::N], h[::N], qkv[:, D:]          # cls rows (row stride N * D); the K | V columns
        xc = b["xc"]
        if not norm1_done:
            layernorm(x, blk["n1w"], blk["n1b"], h, cap * N, D, D, D, count_dev=count, rows_per_count=N)
        linear(h, blk["wkv"], blk["bkv"], b["kv"], m_dev=count, m_mul=N)
        linear(b["hc"], blk["wq"], blk["bq"], b["tq"], m_dev=count, m_mul=1)
        attention_cls(b["tq"], qkv, cap, N, H, b["to"], r_dev=count)
        linear(b["to"], blk["wproj"], blk["bproj"], xc, flags=EPI_RES_F32, m_dev=count, m_mul=1)
        layernorm(x, blk["n2w"], blk["n2b"], b["th"], cap, D, N * D, D, count_dev=count, rows_per_count=1)
        linear(b["th"], blk["wfc1"], blk["bfc1"], b["tg"], flags=EPI_GELU, m_dev=count, m_mul=1)
        linear(b["tg"], blk["wfc2"], blk["bfc2"], xc, flags=EPI_RES_F32, m_dev=count, m_mul=1)

    def _blocks_mxfp8(self, b: dict, cap: int, count: Optional[torch.Tensor]):
        """Block linears in MXFP8.  Operand hand-offs: LayerNorm writes the qkv / fc1 operand directly, the fc1 epilogue
        writes the fc2 operand directly (GELU output never exists in bf16 in HBM), attention writes the proj operand
        directly: no separate quantisation pass is left."""
        D, N = self.D, self.N
        x = b["x"]
        hq, hs, gq, gs = b["q"], b["qs"], b["gq"], b["gs"]
        rows = cap * N
        for blk in self.blocks:
            layernorm_mxfp8(x, blk["n1w"], blk["n1b"], hq, hs, rows, D, D, count_dev=count, rows_per_count=N)
            if self.fp8_attn:                            # the qkv product stays MXFP8: attention_fp8 consumes these bytes
                linear_mxfp8_q(hq, hs, blk["wqkv_q"], blk["wqkv_s"], blk["bqkv"], b["qkv8"], b["qkv8s"], m_dev=count, m_mul=N)
            else:
                linear_mxfp8(hq, hs, blk["wqkv_q"], blk["wqkv_s"], blk["bqkv"], b["qkv"], m_dev=count, m_mul=N)
            self._attention(b, cap, count, mx=True)
            linear_mxfp8(hq, hs, blk["wproj_q"], blk["wproj_s"], blk["bproj"], x, flags=EPI_RES_F32, m_dev=count, m_mul=N)
            layernorm_mxfp8(x, blk["n2w"], blk["n2b"], hq, hs, rows, D, D, count_dev=count, rows_per_count=N)
            linear_mxfp8_q(hq, hs, blk["wfc1_q"], blk["wfc1_s"], blk["bfc1"], gq, gs, flags=EPI_GELU, m_dev=count, m_mul=N)
            linear_mxfp8(gq, gs, blk["wfc2_q"], blk["wfc2_s"], blk["bfc2"], x, flags=EPI_RES_F32, m_dev=count, m_mul=N)

    def head(self, feats: torch.Tensor, cap: int, logits: torch.Tensor, labels: torch.Tensor, scale: float = 1.0,
             accumulate: bool = False, count: Optional[torch.Tensor] = None):
        wrapper_head(feats, self.fc1w, self.fc1b, self.fc2w, self.fc2b, cap, self.nc, logits, labels, scale, accumulate,
                     r_dev=count)
