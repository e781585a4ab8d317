"""Detector training step on the MI355X path (the ultralytics trainer behind
`YOLO(pt).train(...)`, utils/trainYolo.py:13-35; BASELINE.json configs[3]).

`YoloTrainer` owns the un-fused YOLOv8 (Conv = conv -> BatchNorm(batch statistics) -> SiLU) as flat fp32
parameter / gradient / momentum buffers plus a bf16 mirror of the conv weights, and replays fixed lists of C-ABI
launches for forward and backward.  torch only owns device memory.  Layout rules:
  * activations and their gradients are NHWC bf16 matrices (rows = B*H*W padded to a multiple of 64 with zero rows,
    channels) - C2f / SPPF / neck concats are channel slices, so "split" and "concat" are views in both directions;
  * every backward op ACCUMULATES into the gradient slice of its input (all gradient buffers are one allocation,
    zeroed once per step), which is what makes multi-consumer tensors (C2f splits, P3/P4/P5 features) correct;
  * a conv's data gradient is a conv of dz with the flipped / transposed weight (zero-inserted dz for stride 2), its
    weight gradient dz^T . im2col(x) runs on the transposing-read GEMM of the ViT trainer (yv_wgrad).

The network's wiring - which block reads which view and writes which - is stated once, in `train_launches`: Block, Concat and Pool
entries that name their buffers.  The trainer derives its parameters, activations and scratch sizes from that list, `forward`
walks it, `backward` walks `train_backward_order` of it, and `yolo_wgrad_shapes` / `yolo_s2_dgrad_shapes` read it.  The order of the
launches is pinned by tests/test_yolo_trainer_trace_cpu.py.
"""
from __future__ import annotations

import functools
import itertools
import math
import re
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import torch

import yvhip as _yv
from . import (OPT_ADAMW, OPT_SGD_NESTEROV, VIEW_ADD, VIEW_COPY, VIEW_PAD, VIEW_UP2, VIEW_UP2_BWD, VIEW_ZERO_INSERT, YvError, axpby,
               blob_nhwc8, bn_act_bwd, bn_act_bwd_finish, bn_act_fwd, conv_view_bnbwd, ema_update, optim_step,
               bn_stats, bn_stats_finish, bn_ws_floats, cast_colsum, colsum_ws_floats, conv_stats_ws_floats, conv_view,
               conv_dgrad_s2, conv_dgrad_s2_route, conv_view_stats, conv_weight_dgrad, detect_loss,
               detect_loss_ws_bytes, im2col3, maxpool5_bwd, mview, require_gpu, sgd_step, sppf_pool, view_op, wgrad, wgrad_conv3,
               wgrad_conv3_gather, grad_clip_record)
from .engines import LAYER_STRIDE, REG_MAX, _env_flag, detect_widths, yolo_conv_keys, yolo_layers

BN_EPS, BN_MOMENTUM = 1e-3, 0.03


def _r64(n: int) -> int:
    return (n + 63) // 64 * 64


CLIP_GRAD_ENV = "YV_YOLO_CLIP_GRAD"


def clip_grad_value(value, env: str = CLIP_GRAD_ENV) -> Optional[float]:
    """The max_norm of global-norm gradient clipping, or None for off.  `value` None: the environment variable `env` (unset, empty
    or 0: off).  A positive number (inf included) is max_norm, 0 is off; anything else - negative, NaN, no number - is an error."""
    if value is None:
        import os
        value = os.environ.get(env, "").strip() or 0.0
    try:
        if isinstance(value, bool):
            raise ValueError
        v = float(value)
    except (TypeError, ValueError):
        raise YvError(f"clip_grad / {env}: {value!r} is no number") from None
    if not v >= 0.0:
        raise YvError(f"clip_grad / {env}: max_norm must be positive (0: off), got {value!r}")
    return v if v > 0.0 else None


# ---- the training network's launch list: entries of three kinds.  Buffers go by name: x0 (the image, 8 channels), out{idx} (a layer's
# output), y{idx} (the concat buffer of a C2f / SPPF block), t{idx}.{j} (a bottleneck's hidden map), cat{idx} (the neck's concat),
# det{s}.{b0,b1,c0,c1} (the head's feature maps) and det{s}.{box,cls} (its f32 logits).  A view is (buffer, channel offset, channels).
class Block(NamedTuple):
    unit: Union[int, Tuple[int, str]]   # what the block is part of: a layer index, or (head scale, "box" / "cls")
    key: str                    # state-dict prefix
    k: int
    stride: int
    bn: bool                    # True: conv -> BatchNorm -> SiLU, bf16 output; False: plain biased conv, f32 output (Detect's last layers)
    src: tuple                  # the input view
    out: tuple                  # the output view
    res_off: Optional[int]      # channel offset in out's buffer of the residual added to the output, None = no residual
    down_in: int                # the input grid is (size // down_in) x (size // down_in)
    down: int                   # the output grid likewise
    cin: int                    # channels as stored (padded to a multiple of 8) ...
    cout: int
    cin_real: int               # ... and as the state dict has them
    cout_real: int
    dgrad: bool                 # the input has a gradient (the stem's, the image, has none)


class Concat(NamedTuple):
    unit: int
    out: str                    # the neck's concat: both sources copied side by side into `out`
    srcs: tuple                 # two (buffer, channel offset in `out`, channels, up); up = 1: nearest-neighbour 2 x upsample of a grid half the size
    down: int


class Pool(NamedTuple):
    unit: int
    buf: str                    # SPPF: three chained 5 x 5 max-pools of channels [0, c) into the three chunks behind them
    c: int
    down: int


@functools.lru_cache(maxsize=None)
def train_launches(scale: str, nc: int = 5) -> tuple:
    """The un-fused training network in forward order (host only): layers in yaml order, a neck C2f as concat, cv1, the bottleneck
    pairs, cv2, SPPF as cv1, pool, cv2, then the head per scale, box branch before class branch."""
    layers = yolo_layers(scale)
    width = {idx: p["cout"] for idx, _, p in layers}
    out: list = []

    def block(unit, key, src, dst, k, stride, down, bn=True, res_off=None, cin_real=None, cout_real=None, dgrad=True):
        out.append(Block(unit, key, k, stride, bn, src, dst, res_off, down // stride, down, src[2], dst[2],
                         src[2] if cin_real is None else cin_real, dst[2] if cout_real is None else cout_real, dgrad))

    for idx, kind, p in layers:
        pre, d, o = f"model.{idx}", LAYER_STRIDE[idx], (f"out{idx}", 0, p["cout"])
        src = (f"out{idx - 1}", 0, p.get("cin"))
        if kind == "stem":
            block(idx, pre, ("x0", 0, 8), o, 3, 2, d, cin_real=3, dgrad=False)
        elif kind == "conv":
            block(idx, pre, src, o, 3, 2, d)
        elif kind == "c2f":
            c, n, y = p["cout"] // 2, p["n"], f"y{idx}"
            if "a" in p:                                # the neck: concat of two layers' outputs, one of them upsampled
                (ia, ua), (ib, ub) = p["a"], p["b"]
                out.append(Concat(idx, f"cat{idx}", ((f"out{ia}", 0, width[ia], ua), (f"out{ib}", width[ia], width[ib], ub)), d))
                src = (f"cat{idx}", 0, p["cin"])
            block(idx, pre + ".cv1", src, (y, 0, 2 * c), 1, 1, d)
            for j in range(n):
                at, t = (1 + j) * c, f"t{idx}.{j}"
                block(idx, pre + f".m.{j}.cv1", (y, at, c), (t, 0, c), 3, 1, d)
                block(idx, pre + f".m.{j}.cv2", (t, 0, c), (y, at + c, c), 3, 1, d, res_off=at if p["add"] else None)
            block(idx, pre + ".cv2", (y, 0, (2 + n) * c), o, 1, 1, d)
        elif kind == "sppf":
            c_, y = p["cin"] // 2, f"y{idx}"
            block(idx, pre + ".cv1", src, (y, 0, c_), 1, 1, d)
            out.append(Pool(idx, y, c_, d))
            block(idx, pre + ".cv2", (y, 0, 4 * c_), o, 1, 1, d)
    ch, c2, c3, ncp = detect_widths(scale, nc)
    for s, fidx in enumerate((15, 18, 21)):
        d, f = LAYER_STRIDE[fidx], (f"out{fidx}", 0, ch[s])
        for branch, cv, w, co, co_real in (("box", "cv2", c2, 4 * REG_MAX, 4 * REG_MAX), ("cls", "cv3", c3, ncp, nc)):
            unit, pre, a = (s, branch), f"model.22.{cv}.{s}", f"det{s}.{branch[0]}"
            block(unit, pre + ".0", f, (a + "0", 0, w), 3, 1, d)
            block(unit, pre + ".1", (a + "0", 0, w), (a + "1", 0, w), 3, 1, d)
            block(unit, pre + ".2", (a + "1", 0, w), (f"det{s}.{branch}", 0, co), 1, 1, d, bn=False, cout_real=co_real)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def train_backward_order(scale: str, nc: int = 5) -> tuple:
    """The entries of train_launches in the order backward() walks them, as groups: the weight gradients of a group's blocks are
    flushed to the side stream behind it.  A unit's entries run back to front (a block's residual gradient is added right behind
    the block, _bwd), and so do the layers, one group each.  The head is the one place that is NOT a plain reversal: it comes
    first, scale 0, 1, 2, one group per scale, in it the box branch back to front, then the class branch.
    The order is part of the result, not a matter of taste: activation gradients accumulate in bf16 into shared slices, so the
    order of the accumulations decides the bits, and the flush points decide what the weight gradients overlap."""
    units = [tuple(g)[::-1] for _, g in itertools.groupby(train_launches(scale, nc), key=lambda e: e.unit)]
    head = [u for u in units if isinstance(u[0].unit, tuple)]
    scales = [sum(g, ()) for _, g in itertools.groupby(head, key=lambda u: u[0].unit[0])]
    return tuple(scales + [u for u in reversed(units) if not isinstance(u[0].unit, tuple)])


@functools.lru_cache(maxsize=None)
def fused_bn_bwd_pairs(scale: str, nc: int = 5) -> Dict[str, str]:
    """{producer key: consumer key} of the BatchNorm blocks whose output gradient is written completely by ONE launch, the data
    gradient of the block that runs right before them in backward() (host only; the wiring's half of YoloTrainer(fused_bn_bwd=True),
    DESIGN.md section 27).  A producer qualifies if exactly one entry of train_launches reads any channel of its output view, that
    entry is a Block whose input view IS that view (no Concat, no Pool, no other block's residual slice) and the producer is the next
    Block train_backward_order runs behind that consumer."""
    launches = train_launches(scale, nc)
    order = [e for group in train_backward_order(scale, nc) for e in group if isinstance(e, Block)]
    nxt = {a.key: b.key for a, b in zip(order, order[1:])}
    overlap = lambda buf, lo, n, view: buf == view[0] and lo < view[1] + view[2] and view[1] < lo + n

    def readers(view):
        for e in launches:
            if isinstance(e, Block):
                if overlap(*e.src, view) or (e.res_off is not None and overlap(e.out[0], e.res_off, e.out[2], view)):
                    yield e
            elif isinstance(e, Concat):
                if any(name == view[0] for name, _, _, _ in e.srcs):
                    yield e
            elif overlap(e.buf, 0, 4 * e.c, view):
                yield e

    pairs = {}
    for p in launches:
        if isinstance(p, Block) and p.bn:
            rd = list(readers(p.out))
            if len(rd) == 1 and isinstance(rd[0], Block) and rd[0].src == p.out and rd[0].dgrad and nxt.get(rd[0].key) == p.key:
                pairs[p.key] = rd[0].key
    return pairs


def _state_dict_order(launches) -> List[Block]:
    """The blocks in the order ultralytics registers them (which the flat parameter buffer follows): forward order, except that a
    C2f's cv2 sits in front of its bottlenecks."""
    blocks = [e for e in launches if isinstance(e, Block)]
    return [e for _, unit in itertools.groupby(blocks, key=lambda e: e.unit) for e in sorted(unit, key=lambda e: ".m." in e.key)]


def _activations(launches) -> List[Tuple[str, int, int]]:
    """(name, grid divisor, channels) of every bf16 activation of the list, in the order the trainer allocates them (which the
    offsets of the gradients in their one allocation follow): unit by unit, in a layer x0, out, y, t.j, cat, in the head as used."""
    dims: Dict[str, list] = {}                          # buffer: [unit that uses it first, grid divisor, channels]
    for e in launches:
        if isinstance(e, Block):
            uses = [(e.src[0], e.src[1] + e.src[2], e.down_in)] + [(e.out[0], e.out[1] + e.out[2], e.down)] * e.bn
        elif isinstance(e, Concat):
            uses = [(e.out, sum(c for _, _, c, _ in e.srcs), e.down)]
        else:
            uses = [(e.buf, 4 * e.c, e.down)]
        for buf, c, down in uses:
            d = dims.setdefault(buf, [e.unit, down, 0])
            d[2] = max(d[2], c)
    rank = lambda name: ("x", "out", "y", "t", "cat", "det").index(re.match("[a-z]+", name).group())
    return [(name, d, c) for _, unit in itertools.groupby(dims.items(), key=lambda kv: kv[1][0])
            for name, (_, d, c) in sorted(unit, key=lambda kv: rank(kv[0]))]


def fused_bn_bwd_plan(scale: str, nc: int, size: int, batch: int, phase_blocks=frozenset()) -> Dict[str, str]:
    """{consumer key: producer key} of the pairs YoloTrainer(fused_bn_bwd=True) fuses at this size and batch (host only): the pairs
    of fused_bn_bwd_pairs whose consumer's data gradient is not a phase launch (`phase_blocks`: the trainer's _phase_blocks; the
    PHASE form takes no sums) and whose route says `use`, i.e. conv_view would not split K for the same call.  The route is reached
    through the package so that a launch trace, which stubs the wrappers this module imports, gets the real answer."""
    launches = train_launches(scale, nc)
    by_key = {e.key: e for e in launches if isinstance(e, Block)}
    width = {name: c for name, _, c in _activations(launches)}
    plan = {}
    for pkey, ckey in fused_bn_bwd_pairs(scale, nc).items():
        c, hin, ld = by_key[ckey], size // by_key[ckey].down_in, width[by_key[ckey].src[0]]
        if ckey in phase_blocks:
            continue
        try:                                            # the data gradient: (batch, hin, hin) x c.cout -> c.cin, stride 1
            use = _yv.conv_bnbwd_route(batch, hin, hin, c.k, 1, c.cout, c.cin, out_ld=ld, res_ld=ld, ldz=by_key[pkey].cout).use
        except YvError:
            use = False
        if use:
            plan[ckey] = pkey
    return plan


def init_yolo_train_state(scale: str = "n", nc: int = 5, seed: int = 42) -> Dict[str, torch.Tensor]:
    """Seeded random UN-FUSED weights in the ultralytics key layout (`*.conv.weight`, `*.bn.{weight,bias,running_mean,
    running_var}`, Detect's `cv2.s.2.{weight,bias}`): there is no network on the box, so benchmarks and smoke tests
    train from this instead of a downloaded `.pt`."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for key, ci, co, k in yolo_conv_keys(scale, nc):
        w = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        if key.endswith(".conv"):
            base = key[:-5]
            sd[base + ".conv.weight"] = w
            sd[base + ".bn.weight"] = torch.ones(co)
            sd[base + ".bn.bias"] = torch.zeros(co)
            sd[base + ".bn.running_mean"] = torch.zeros(co)
            sd[base + ".bn.running_var"] = torch.ones(co)
        else:
            sd[key + ".weight"] = w
            # ultralytics Detect.bias_init: box branch 1.0, class branch log(5 / nc / (640 / stride)^2)
            s_idx = int(key.split(".")[3])
            sd[key + ".bias"] = (torch.full((co,), 1.0) if ".cv2." in key else
                                 torch.full((co,), math.log(5 / nc / (640 / (8 << s_idx)) ** 2)))
    return sd


def yolo_wgrad_shapes(scale: str, nc: int, size: int = 640, batch: int = 16,
                      implicit: bool = True) -> List[Tuple[str, int, int, int, int]]:
    """(key, T, N, K, pitch) of every weight-gradient product of a YoloTrainer step (host only): dW (N, K) over T tokens,
    channels padded to 8, T to 64.  pitch > 0: a 3x3 / stride 1 layer on the zero-padded pixel grid of that row pitch
    (wgrad_conv3; `implicit`), 0: wgrad on the activation (1x1) or on its im2col."""
    out = []
    for e in _state_dict_order(train_launches(scale, nc)):
        h = size // e.down
        pitch = h + 2 if e.k == 3 and e.stride == 1 and implicit else 0
        out.append((e.key + (".conv" if e.bn else ""), _r64(batch * pitch * pitch if pitch else batch * h * h), e.cout,
                    e.k * e.k * e.cin, pitch))
    return out


def yolo_s2_dgrad_shapes(scale: str, size: int = 640) -> List[Tuple[str, int, int, int]]:
    """(key, Hin, Cin, Cout) of every stride-2 convolution of a YoloTrainer step that has a data gradient (host only): model.1, 3,
    5, 7, 16, 19 - the stem's input is the image."""
    return [(e.key, 2 * (size // e.down), e.cin, e.cout)
            for e in train_launches(scale) if isinstance(e, Block) and e.stride == 2 and e.dgrad]


class _Act:
    """(B,H,W,C) bf16 activation + its gradient, stored as (rows padded to 64, C)."""

    def __init__(self, dev: torch.device, B: int, H: int, W: int, Cn: int):
        self.B, self.H, self.W, self.C = B, H, W, Cn
        self.T = B * H * W
        self.buf = torch.zeros((_r64(self.T), Cn), dtype=torch.bfloat16, device=dev)
        self.grad: Optional[torch.Tensor] = None            # a slice of the trainer's one gradient allocation

    def v(self, off: int = 0, c: Optional[int] = None):
        return mview(self.buf, off, self.C - off if c is None else c)

    def g(self, off: int = 0, c: Optional[int] = None):
        return mview(self.grad, off, self.C - off if c is None else c)


class _Block:
    """One Conv(+BN+SiLU) (bn=True) or plain biased conv (Detect's last layers)."""

    def __init__(self, tr: "YoloTrainer", e: Block):
        self.e, self.key, self.cin, self.cout, self.k, self.s, self.bn = e, e.key, e.cin, e.cout, e.k, e.stride, e.bn
        self.cin_real, self.cout_real, self.taps = e.cin_real, e.cout_real, e.k * e.k
        self.w = tr._param(e.key + (".conv.weight" if e.bn else ".weight"), e.cout * self.taps * e.cin, "w")
        if e.bn:                                 # ultralytics groups: conv weights (decay) / BatchNorm weights / all biases
            self.gamma = tr._param(e.key + ".bn.weight", e.cout, "bnw")
            self.beta = tr._param(e.key + ".bn.bias", e.cout, "bias")
        else:
            self.bias = tr._param(e.key + ".bias", e.cout, "bias")

    def bind(self, tr: "YoloTrainer"):
        """The operands the entry names, resolved once: x / dx the input view and its gradient (None: no data gradient), x_buf,
        x_off the input rows as the weight gradient takes them, y / dy the output view and its gradient (a plain block: the f32
        logits and the loss kernel's gradient of them), res / dres the residual view and its gradient; and the block's own slices
        of the flat buffers (every allocation lives as long as the trainer), so that a step slices nothing again."""
        e, key, src = self.e, self.key, tr.act[self.e.src[0]]
        self.w16, self.dw, self.dzv = tr.w16(self), tr.gr(self.w).view(self.cout, self.taps * self.cin), mview(tr.dz[key])
        self.x_buf, self.x_off = src.buf, e.src[1]
        self.x, self.dx = src.v(*e.src[1:]), src.g(*e.src[1:]) if e.dgrad else None
        self.res = self.dres = None
        if e.bn:
            dst, self.zv = tr.act[e.out[0]], mview(tr.z[key])
            self.stat, self.run = (tr.mean[key], tr.rstd[key]), (tr.run_mean[key], tr.run_var[key])
            self.affine, self.daffine = (tr.p(self.gamma), tr.p(self.beta)), (tr.gr(self.gamma), tr.gr(self.beta))
            self.y, self.dy = dst.v(*e.out[1:]), dst.g(*e.out[1:])
            if e.res_off is not None:
                self.res, self.dres = dst.v(e.res_off, e.out[2]), dst.g(e.res_off, e.out[2])
        else:
            s, branch = e.unit
            self.bias_p, self.dbias = tr.p(self.bias), tr.gr(self.bias)
            self.y, self.dy = mview(tr.det_out[e.out[0]]), tr.det_out[f"det{s}.d{branch}"]


class YoloTrainer:
    def __init__(self, state: Dict[str, torch.Tensor], scale: str = "n", nc: int = 5, size: int = 640, batch: int = 16,
                 lr: float = 1e-4, momentum: float = 0.937, weight_decay: float = 5e-4, device: str = "cuda:0",
                 optimizer: str = "sgd", ema: bool = False, ema_decay: float = 0.9999, ema_tau: float = 2000.0,
                 overlap_wgrad: bool = True, implicit_wgrad: bool = True, narrow_wgrad: Optional[bool] = None,
                 fused_bn_stats: Optional[bool] = None, phase_dgrad: Optional[bool] = None, gather_wgrad: Optional[bool] = None,
                 fused_bn_bwd: Optional[bool] = None, clip_grad: Optional[float] = None):
        require_gpu()
        if size % 32:
            raise YvError("input size must be a multiple of 32")
        # opt-in: clip the global L2 norm of the gradients to this max_norm ahead of every update (torch's clip_grad_norm_; the
        # published trainer: 10.0) and skip an update whose norm is not finite, all on the device; DESIGN.md section 28
        self.clip_grad = clip_grad_value(clip_grad)
        self.scale, self.nc, self.size, self.B, self.dev = scale, nc, size, batch, torch.device(device)
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.overlap_wgrad, self.s_w, self._pending = overlap_wgrad, None, []
        self.implicit_wgrad = implicit_wgrad               # 3x3 / stride 1 weight gradients without an im2col buffer
        # opt-in: weight gradients on the N tile wgrad_route picks (32 / 64 x 256 for few output channels); off = yv_wgrad's 128 x 128
        self.narrow_wgrad = _env_flag(narrow_wgrad, "YV_YOLO_NARROW_WGRAD")
        self._wgrad_tile = 0 if self.narrow_wgrad else None
        # opt-in: the forward's BatchNorm batch statistics from the convolution's epilogue (yv_conv2d_stats + yv_bn_stats_finish)
        # in place of a pass over z (yv_bn_stats); DESIGN.md section 22
        self.fused_bn_stats = _env_flag(fused_bn_stats, "YV_YOLO_FUSED_BN_STATS")
        # opt-in: the data gradient of the stride-2 convolutions by parity phase (yv_conv2d_dgrad_s2) in place of zero insertion +
        # a stride-1 convolution, for the blocks whose route says so (_alloc_buffers); DESIGN.md section 24
        self.phase_dgrad = _env_flag(phase_dgrad, "YV_YOLO_PHASE_DGRAD")
        self._phase_blocks: set = set()
        # opt-in: the weight gradient of the 3 x 3 / stride-2 convolutions with gathered source addresses (yv_wgrad_conv3_gather)
        # in place of im2col + wgrad, for the blocks whose route says so (_alloc_buffers); needs implicit_wgrad (without it the
        # trainer is the im2col statement); DESIGN.md section 26
        self.gather_wgrad = _env_flag(gather_wgrad, "YV_YOLO_GATHER_WGRAD")
        self._gather_blocks: set = set()
        # opt-in: the two reductions of a BatchNorm block's backward from the epilogue of the data gradient that writes the block's
        # output gradient (yv_conv2d_bnbwd + yv_bn_act_bwd_finish) in place of bn_act_bwd's pass over da and z, for the pairs of
        # fused_bn_bwd_plan (asked once, at construction, and only with the flag on); DESIGN.md section 27
        self.fused_bn_bwd = _env_flag(fused_bn_bwd, "YV_YOLO_FUSED_BN_BWD")
        self._bnbwd_of: Dict[str, str] = {}               # consumer key -> producer key
        self._bnbwd_producers: set = set()
        self.bn_bwd_ws: Optional[torch.Tensor] = None      # the pairs' tile partials (not self.ws: the consumer's own bn_act_bwd uses that)
        if optimizer not in ("sgd", "sgd_nesterov", "adamw"):
            raise YvError("optimizer must be 'sgd', 'sgd_nesterov' or 'adamw'")
        self.optimizer, self.use_ema, self.ema_decay, self.ema_tau = optimizer, ema, ema_decay, ema_tau
        self.ncp = (nc + 7) // 8 * 8
        self._pspecs: List[Tuple[str, int, str]] = []
        self.layers = yolo_layers(scale)
        self.launches, self._backward_order = train_launches(scale, nc), train_backward_order(scale, nc)
        self.blocks: List[_Block] = [_Block(self, e) for e in _state_dict_order(self.launches)]
        self.block: Dict[str, _Block] = {b.key: b for b in self.blocks}
        self._alloc_params(state)
        self._alloc_buffers()
        self.step_count = 0
        self.loss_out = torch.zeros(4, device=self.dev)
        self._loss_ws: Dict[int, torch.Tensor] = {}
        from .dist import BucketReducer
        self.reducer = BucketReducer(self.G, 1 << 62)            # 12-45 MB of gradients: one all-reduce after backward
        self.clip_ws = self.clip_rec = self.clip_skipped = None
        if self.clip_grad is not None:
            self.clip_ws = torch.zeros(max(_yv.grad_clip_ws_bytes(self.n_param), 16), dtype=torch.uint8, device=self.dev)
            self.clip_rec = torch.zeros(4, device=self.dev)       # sum of squares, norm, coefficient, grad_scale * coefficient
            self.clip_skipped = torch.zeros(1, dtype=torch.int32, device=self.dev)

    @property
    def grad_norm_record(self) -> torch.Tensor:
        """The device record of the last optimizer_step (yv_grad_clip_record's four floats; no copy)."""
        if self.clip_rec is None:
            raise YvError("trainer was built without clip_grad")
        return self.clip_rec

    @property
    def skipped_steps(self) -> torch.Tensor:
        """The device counter (1 i32) of the updates skipped for a gradient norm that was not finite."""
        if self.clip_skipped is None:
            raise YvError("trainer was built without clip_grad")
        return self.clip_skipped

    # ------------------------------------------------------------------ parameters
    def _param(self, name: str, n: int, group: str) -> int:
        self._pspecs.append((name, n, group))
        return len(self._pspecs) - 1

    def _alloc_params(self, state: Dict[str, torch.Tensor]):
        order = [i for g in ("w", "bnw", "bias") for i, s in enumerate(self._pspecs) if s[2] == g]
        self.off: Dict[int, Tuple[int, int]] = {}
        self.group: Dict[str, Tuple[int, int]] = {}
        pos = 0
        for i in order:
            n = (self._pspecs[i][1] + 7) // 8 * 8            # 32-byte aligned segments
            self.off[i] = (pos, self._pspecs[i][1])
            g = self._pspecs[i][2]
            lo = self.group[g][0] if g in self.group else pos
            pos += n
            self.group[g] = (lo, pos)
        self.n_weight = self.group["w"][1]
        self.n_param = pos
        host = torch.zeros(pos, dtype=torch.float32)
        for b in self.blocks:
            o, n = self.off[b.w]
            wkey = b.key + (".conv.weight" if b.bn else ".weight")
            w = state[wkey].float()
            if tuple(w.shape) != (b.cout_real, b.cin_real, b.k, b.k):
                raise YvError(f"{wkey} has shape {tuple(w.shape)}, expected {(b.cout_real, b.cin_real, b.k, b.k)}")
            wp = torch.zeros(b.cout, b.k, b.k, b.cin)
            wp[:b.cout_real, :, :, :b.cin_real] = w.permute(0, 2, 3, 1)                  # (Cout, ky, kx, Cin)
            host[o:o + n] = wp.reshape(-1)
            if b.bn:
                for pid, suffix in ((b.gamma, ".bn.weight"), (b.beta, ".bn.bias")):
                    o2, n2 = self.off[pid]
                    host[o2:o2 + n2] = state[b.key + suffix].float()
            else:
                o2, n2 = self.off[b.bias]
                host[o2:o2 + b.cout_real] = state[b.key + ".bias"].float()
        self.P = host.to(self.dev)
        self.G = torch.zeros_like(self.P)
        self.Mo = torch.zeros_like(self.P)
        self.P16 = self.P[:self.n_weight].to(torch.bfloat16)
        self.V: Optional[torch.Tensor] = None                     # AdamW second moments (allocated on first use)
        # running statistics: one flat buffer (mean | var per block) so the EMA is a single launch
        n_rs = sum(2 * b.cout for b in self.blocks if b.bn)
        rs_host = torch.zeros(n_rs)
        self._rs_off: Dict[str, int] = {}
        pos = 0
        for b in self.blocks:
            if b.bn:
                self._rs_off[b.key] = pos
                rs_host[pos:pos + b.cout] = state[b.key + ".bn.running_mean"].float()
                rs_host[pos + b.cout:pos + 2 * b.cout] = state[b.key + ".bn.running_var"].float()
                pos += 2 * b.cout
        self.RS = rs_host.to(self.dev)
        self.run_mean = {b.key: self.RS[self._rs_off[b.key]:self._rs_off[b.key] + b.cout] for b in self.blocks if b.bn}
        self.run_var = {b.key: self.RS[self._rs_off[b.key] + b.cout:self._rs_off[b.key] + 2 * b.cout] for b in self.blocks if b.bn}
        self.P_ema = self.P.clone() if self.use_ema else None
        self.RS_ema = self.RS.clone() if self.use_ema else None
        self.ema_updates = 0
        self.G_acc: Optional[torch.Tensor] = None
        self.accumulated = 0

    def p(self, pid: int) -> torch.Tensor:
        o, n = self.off[pid]
        return self.P[o:o + n]

    def gr(self, pid: int) -> torch.Tensor:
        o, n = self.off[pid]
        return self.G[o:o + n]

    def w16(self, b: _Block) -> torch.Tensor:
        o, n = self.off[b.w]
        return self.P16[o:o + n]

    def state_dict(self, ema: bool = False) -> Dict[str, torch.Tensor]:
        """Un-fused ultralytics key layout, fp32, on the host; ema=True returns the ModelEMA copy (what ultralytics saves)."""
        if ema and not self.use_ema:
            raise YvError("trainer was built without ema=True")
        return self._unpack((self.P_ema if ema else self.P).cpu(), (self.RS_ema if ema else self.RS).cpu())

    def grads(self) -> Dict[str, torch.Tensor]:
        """Gradients in the layout of state_dict() (tests)."""
        return self._unpack(self.G.cpu())

    def _unpack(self, flat: torch.Tensor, rs: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """A host copy of a flat buffer in P's layout (and of the running statistics) under the un-fused ultralytics keys."""
        sd: Dict[str, torch.Tensor] = {}
        for b in self.blocks:
            o, n = self.off[b.w]
            w = flat[o:o + n].view(b.cout, b.k, b.k, b.cin)[:b.cout_real, :, :, :b.cin_real].permute(0, 3, 1, 2).contiguous()
            if b.bn:
                sd[b.key + ".conv.weight"] = w
                for pid, suffix in ((b.gamma, ".bn.weight"), (b.beta, ".bn.bias")):
                    o2, n2 = self.off[pid]
                    sd[b.key + suffix] = flat[o2:o2 + n2].clone()
                if rs is not None:
                    ro = self._rs_off[b.key]
                    sd[b.key + ".bn.running_mean"] = rs[ro:ro + b.cout].clone()
                    sd[b.key + ".bn.running_var"] = rs[ro + b.cout:ro + 2 * b.cout].clone()
            else:
                sd[b.key + ".weight"] = w
                o2, _ = self.off[b.bias]
                sd[b.key + ".bias"] = flat[o2:o2 + b.cout_real].clone()
        return sd

    # ------------------------------------------------------------------ buffers
    def _alloc_buffers(self):
        B, S, dev = self.B, self.size, self.dev
        self.act: Dict[str, _Act] = {name: _Act(dev, B, S // down, S // down, c) for name, down, c in _activations(self.launches)}
        self.x0, self.out = self.act["x0"], {idx: self.act[f"out{idx}"] for idx, _, _ in self.layers}
        # one allocation for every activation gradient (zeroed once per step)
        total = sum(a.buf.numel() for a in self.act.values())
        self.grad_flat = torch.zeros(total, dtype=torch.bfloat16, device=dev)
        pos = 0
        for a in self.act.values():
            n = a.buf.numel()
            a.grad = self.grad_flat[pos:pos + n].view(a.buf.shape)
            pos += n
        self.det_out: Dict[str, torch.Tensor] = {}                # the head's f32 logits and the loss kernel's gradient of them
        self.z, self.dz, self.mean, self.rstd = {}, {}, {}, {}   # by block key: pre-activation, its gradient, the batch statistics
        self.geom: Dict[str, Tuple[int, int]] = {}                # by block key: (input grid, output grid)
        ws_f, wd_n, col_n, zi_n, xp_n, dzp_n = 0, 0, 0, 0, 0, 0
        for b in self.blocks:
            hin, hout = self.geom[b.key] = S // b.e.down_in, S // b.e.down
            T = B * hout * hout
            if b.bn:
                self.z[b.key] = torch.zeros((_r64(T), b.cout), dtype=torch.bfloat16, device=dev)
                self.mean[b.key] = torch.zeros(b.cout, device=dev)
                self.rstd[b.key] = torch.zeros(b.cout, device=dev)
                ws_f = max(ws_f, bn_ws_floats(T, b.cout))
                if self.fused_bn_stats:
                    ws_f = max(ws_f, conv_stats_ws_floats(T, b.cout))
            else:
                s, branch = b.e.unit
                for name in (branch, "d" + branch):                # det{s}.box / .cls, det{s}.dbox / .dcls
                    self.det_out[f"det{s}.{name}"] = torch.zeros((T, b.cout), device=dev)
                ws_f = max(ws_f, colsum_ws_floats(T, b.cout))
            self.dz[b.key] = torch.zeros((_r64(T), b.cout), dtype=torch.bfloat16, device=dev)
            wd_n = max(wd_n, b.cout * b.taps * b.cin)
            if b.k == 3 and b.s == 1 and self.implicit_wgrad:
                hp = hin + 2                                   # operands of yv_wgrad_conv3 live on the zero-padded grid
                tpp = _r64(B * hp * hp)
                xp_n = max(xp_n, (tpp + 2 * (hp + 1)) * b.cin)
                dzp_n = max(dzp_n, tpp * b.cout)
            elif b.k == 3 and self.gather_wgrad and self.implicit_wgrad and self._gather_eligible(b, hin):
                self._gather_blocks.add(b.key)
            elif b.k == 3:
                col_n = max(col_n, _r64(T) * 9 * b.cin)
            if b.s == 2 and self.phase_dgrad and self._phase_eligible(b, hin):
                self._phase_blocks.add(b.key)
            elif b.s == 2:
                zi_n = max(zi_n, B * hin * hin * b.cout)
        self.ws = torch.zeros(max(ws_f, 16), device=dev)
        self.wd_buf = torch.zeros(max(wd_n, 8), dtype=torch.bfloat16, device=dev)
        self.col = torch.zeros(max(col_n, 8), dtype=torch.bfloat16, device=dev)
        self.zi = torch.zeros(max(zi_n, 8), dtype=torch.bfloat16, device=dev)
        self.xp = torch.zeros(max(xp_n, 8), dtype=torch.bfloat16, device=dev)       # zero-initialised: its margins are read
        self.dzp = torch.zeros(max(dzp_n, 8), dtype=torch.bfloat16, device=dev)
        if self.fused_bn_bwd:
            bw_f = 0
            self._bnbwd_of = fused_bn_bwd_plan(self.scale, self.nc, S, B, frozenset(self._phase_blocks))
            self._bnbwd_producers = set(self._bnbwd_of.values())
            for pkey in self._bnbwd_producers:
                hout = self.geom[pkey][1]
                bw_f = max(bw_f, _yv.conv_bnbwd_ws_floats(B * hout * hout, self.block[pkey].cout))
            self.bn_bwd_ws = torch.zeros(max(bw_f, 16), device=dev)
        for b in self.blocks:
            b.bind(self)

    def _phase_eligible(self, b: _Block, hin: int) -> bool:
        """The route's answer for this block's data gradient (asked once, at construction): eligible and not measured slower."""
        try:
            return conv_dgrad_s2_route(self.B, hin, hin, b.k, b.cin, b.cout).use
        except YvError:
            return False

    def _gather_eligible(self, b: _Block, hin: int) -> bool:
        """The route's answer for this block's weight gradient (asked once, at construction, and only with the flag on).  The
        route is reached through the package so that a launch trace, which stubs the wrappers this module imports, gets the real
        answer."""
        try:
            return _yv.wgrad_conv3_gather_route(self.B, hin, hin, b.s, b.cin, b.cout,
                                                128 if self._wgrad_tile is None else self._wgrad_tile)[1]
        except YvError:
            return False

    # ------------------------------------------------------------------ one block, forward / backward
    def _fwd(self, b: _Block):
        hout = self.geom[b.key][1]
        if not b.bn:                                            # Detect's last 1 x 1: biased, f32 logits
            conv_view(b.x, self.B, hout, hout, b.k, b.s, b.w16, b.cout, b.y, bias=b.bias_p, out_f32=True)
            return
        T = self.B * hout * hout
        if self.fused_bn_stats:
            conv_view_stats(b.x, self.B, hout, hout, b.k, b.s, b.w16, b.cout, b.zv, self.ws)
            bn_stats_finish(self.ws, T, *b.stat, *b.run, BN_EPS, BN_MOMENTUM)
        else:
            conv_view(b.x, self.B, hout, hout, b.k, b.s, b.w16, b.cout, b.zv)
            bn_stats(b.zv, T, *b.stat, *b.run, self.ws, BN_EPS, BN_MOMENTUM)
        bn_act_fwd(b.zv, T, *b.stat, *b.affine, b.y, res=b.res)

    def _bwd(self, b: _Block, da=None):
        """From the gradient of the block's output (b.dy; da: a caller's gradient of a plain block's logits in its place) to the
        block's parameter gradients and, accumulated, the gradients of its input (b.dx) and of its residual (b.dres)."""
        hin, hout = self.geom[b.key]
        T = self.B * hout * hout
        if b.bn and b.key in self._bnbwd_producers:             # the sums are in bn_bwd_ws: the consumer's data gradient left them
            bn_act_bwd_finish(b.dy, b.zv, T, *b.stat, *b.affine, *b.daffine, b.dzv, self.bn_bwd_ws)
        elif b.bn:
            bn_act_bwd(b.dy, b.zv, T, *b.stat, *b.affine, *b.daffine, b.dzv, self.ws)
        else:                                                   # the f32 loss gradient (T, cout): cast + bias gradient
            cast_colsum(b.dy if da is None else da, self.dz[b.key], b.dbias, self.ws)
        if self.overlap_wgrad:
            self._pending.append((b, b.x_buf, b.x_off))         # weight gradients run on the side stream (_flush_wgrads)
        else:
            self._wgrad_block(b, b.x_buf, b.x_off)
        if b.dx is not None:
            wd = self.wd_buf[:b.cin * b.taps * b.cout]
            conv_weight_dgrad(b.w16, b.cout, b.taps, b.cin, wd)
            if b.key in self._phase_blocks:
                conv_dgrad_s2(b.dzv, self.B, hout, hout, wd, b.cin, b.cout, b.dx, res=b.dx)
            else:
                if b.s == 1:
                    src = b.dzv
                else:
                    zi = self.zi[:self.B * hin * hin * b.cout].view(self.B * hin * hin, b.cout)
                    view_op(VIEW_ZERO_INSERT, b.dzv, mview(zi), self.B, hout, hout)
                    src = mview(zi)
                if b.key in self._bnbwd_of:                     # b.dx is the producer's whole output gradient, written here only
                    p = self.block[self._bnbwd_of[b.key]]
                    conv_view_bnbwd(src, self.B, hin, hin, b.k, 1, wd.view(b.cin, b.taps * b.cout), b.cin, b.dx, p.zv, *p.stat, *p.affine,
                                    self.bn_bwd_ws, res=b.dx)
                else:
                    conv_view(src, self.B, hin, hin, b.k, 1, wd.view(b.cin, b.taps * b.cout), b.cin, b.dx, res=b.dx)
        if b.dres is not None:                                  # behind the block, in front of the one that wrote the residual
            view_op(VIEW_ADD, b.dy, b.dres, self.B, hout, hout)

    def _wgrad_block(self, b: _Block, x_buf: torch.Tensor, x_off: int):
        hin, hout = self.geom[b.key]
        T = self.B * hout * hout
        Tp = _r64(T)
        dz, dw = self.dz[b.key], b.dw
        if b.k == 1:
            wgrad(dz, x_buf[:, x_off:x_off + b.cin], dw, T=Tp, tile_n=self._wgrad_tile)
        elif b.s == 1 and self.implicit_wgrad:
            # no im2col: both operands are copied once onto the zero-padded pixel grid, where every tap is a constant row
            # offset and the three taps of a kernel row are contiguous (yv_wgrad_conv3)
            hp = hin + 2
            tpad = self.B * hp * hp
            tpp, mg = _r64(tpad), hp + 1
            xp = self.xp[mg * b.cin:(mg + tpp) * b.cin].view(tpp, b.cin)
            view_op(VIEW_PAD, mview(x_buf, x_off, b.cin), mview(xp), self.B, hin, hin)
            dzp = self.dzp[:tpp * b.cout].view(tpp, b.cout)
            view_op(VIEW_PAD, b.dzv, mview(dzp), self.B, hout, hout)
            if tpp != tpad:
                dzp[tpad:].zero_()
            wgrad_conv3(dzp, xp, dw, tpp, hp, tile_n=self._wgrad_tile)
        elif b.key in self._gather_blocks:
            # no im2col either: the kernel computes each tap's source pixel and reads dz and x in place (yv_wgrad_conv3_gather)
            wgrad_conv3_gather(dz, mview(x_buf, x_off, b.cin), dw, self.B, hin, hin, b.s, tile_n=self._wgrad_tile)
        else:
            col = self.col[:Tp * 9 * b.cin].view(Tp, 9 * b.cin)
            if Tp != T:
                col[T:].zero_()
            im2col3(mview(x_buf, x_off, b.cin), self.B, hin, hin, b.s, col)
            wgrad(dz, col, dw, T=Tp, tile_n=self._wgrad_tile)

    def _flush_wgrads(self):
        """The weight gradients of the blocks back-propagated since the last flush go to a second HIP stream: nothing on
        the data-gradient chain depends on them (only the optimiser does), and the chain's kernels leave CUs idle.  Hazards:
        dz of a block is written once per step (main stream, before the event) and activations are read-only in backward;
        the im2col scratch is private to the side stream; gradient slices are disjoint."""
        if not self._pending:
            return
        if self.s_w is None:
            self.s_w = torch.cuda.Stream()
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(self.s_w):
            self.s_w.wait_event(ev)
            for b, x_buf, x_off in self._pending:
                self._wgrad_block(b, x_buf, x_off)
        self._pending = []

    # ------------------------------------------------------------------ forward
    def forward(self, images: torch.Tensor):
        """images (B,S,S,3) u8 on the device -> per scale (box logits (B*h*h, 64) f32, class logits (B*h*h, ncp) f32)."""
        B, S = self.B, self.size
        if images.dtype != torch.uint8 or tuple(images.shape) != (B, S, S, 3) or not images.is_cuda:
            raise YvError(f"images must be ({B},{S},{S},3) uint8 on the device")
        blob_nhwc8(images.contiguous(), self.x0.buf)
        for e in self.launches:
            if isinstance(e, Block):
                self._fwd(self.block[e.key])
            elif isinstance(e, Concat):
                for name, at, c, up in e.srcs:
                    src = self.act[name]
                    view_op(VIEW_UP2 if up else VIEW_COPY, src.v(), self.act[e.out].v(at, c), B, src.H, src.W)
            else:
                y = self.act[e.buf]
                sppf_pool(y.buf[:y.T].view(B, y.H, y.W, y.C), e.c)
        return [(self.det_out[f"det{s}.box"], self.det_out[f"det{s}.cls"]) for s in range(3)]

    # ------------------------------------------------------------------ backward
    def backward(self, dlogits=None):
        """dlogits: per scale (d box (T,64) f32, d cls (T,ncp) f32); default: the buffers the loss kernel filled."""
        B = self.B
        da = {} if dlogits is None else {f"det{s}.{name}": t for s, pair in enumerate(dlogits) for name, t in zip(("box", "cls"), pair)}
        self.grad_flat.zero_()
        for group in self._backward_order:
            for e in group:
                if isinstance(e, Block):
                    self._bwd(self.block[e.key], da.get(e.out[0]))
                elif isinstance(e, Concat):
                    for name, at, c, up in e.srcs:
                        src = self.act[name]
                        view_op(VIEW_UP2_BWD if up else VIEW_ADD, self.act[e.out].g(at, c), src.g(), B, src.H, src.W)
                else:
                    y, c = self.act[e.buf], e.c
                    for q in (2, 1, 0):                       # p_{q+1} = maxpool(p_q)
                        maxpool5_bwd(y.v(q * c, c), y.g((q + 1) * c, c), y.g(q * c, c), B, y.H, y.W)
            self._flush_wgrads()
        if self.s_w is not None:
            torch.cuda.current_stream().wait_stream(self.s_w)      # every weight gradient is in G before the caller goes on

    # ------------------------------------------------------------------ loss / step
    def loss(self, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_counts: torch.Tensor, gains=(7.5, 0.5, 1.5)):
        """v8 detection loss of the last forward; fills the d-logit buffers backward() consumes.
        gt_boxes (B,G,4) f32 xyxy input pixels, gt_labels (B,G) i32, gt_counts (B) i32, all on the device.
        Returns the device tensor {total*B, box, cls, dfl} (no host sync)."""
        B, G = self.B, gt_boxes.shape[1]
        if tuple(gt_boxes.shape) != (B, G, 4) or tuple(gt_labels.shape) != (B, G) or tuple(gt_counts.shape) != (B,):
            raise YvError("targets must be gt_boxes (B,G,4), gt_labels (B,G), gt_counts (B)")
        A = sum((self.size // st) ** 2 for st in (8, 16, 32))
        if G not in self._loss_ws:
            self._loss_ws[G] = torch.zeros(detect_loss_ws_bytes(B, A, G), dtype=torch.uint8, device=self.dev)
        box, cls, dbox, dcls = ([self.det_out[f"det{s}.{name}"] for s in range(3)] for name in ("box", "cls", "dbox", "dcls"))
        detect_loss(box, cls, dbox, dcls, B, self.size, self.nc, self.ncp, gt_boxes, gt_labels, gt_counts, self.loss_out,
                    self._loss_ws[G], gains)
        return self.loss_out

    def step(self, images: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_counts: torch.Tensor,
             lr: Optional[float] = None, accumulate: int = 1, lrs: Optional[Dict[str, float]] = None,
             momentum: Optional[float] = None):
        """forward -> loss -> backward -> [every `accumulate` calls: data-parallel SUM all-reduce (mean folded into the
        update) -> optimiser -> EMA].  `lrs` gives per-group learning rates ({'w','bnw','bias'}: warm-up treats biases
        differently), `momentum` overrides momentum / beta1 for this step."""
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.forward(images)
        loss = self.loss(gt_boxes, gt_labels, gt_counts)
        self.backward()
        if accumulate > 1:
            if self.G_acc is None:
                self.G_acc = torch.zeros_like(self.G)
            if self.accumulated == 0:
                self.G_acc.copy_(self.G)
            else:
                axpby(self.G_acc, self.G, 1.0, 1.0)
            self.accumulated += 1
            if self.accumulated < accumulate:
                return loss
            self.G.copy_(self.G_acc)
            self.accumulated = 0
        self.reducer.reset()
        self.reducer.finish()
        self.optimizer_step(lr, grad_scale=1.0 / world, lrs=lrs, momentum=momentum)
        return loss

    # ------------------------------------------------------------------ optimiser
    def optimizer_step(self, lr: Optional[float] = None, grad_scale: float = 1.0, lrs: Optional[Dict[str, float]] = None,
                       momentum: Optional[float] = None):
        """One update of every parameter group (ultralytics: weight decay on conv weights only; BatchNorm weights and
        all biases undecayed) with torch.optim.SGD / SGD(nesterov) / AdamW semantics, then the ModelEMA update.
        With clip_grad: one grad_clip_record over all of G first (its padded positions are zero), and every group takes its
        gradient scale from that record on the device - no host synchronisation.  A record whose norm is not finite makes the
        three updates no-ops; step_count and the EMA still advance (unlike an update a loss scaler skips, which the published
        trainer does not count: here the host never learns of the skip, and the EMA of unchanged weights moves towards them)."""
        lr = self.lr if lr is None else lr
        mom = self.momentum if momentum is None else momentum
        self.step_count += 1
        t = self.step_count
        if self.clip_grad is not None:
            grad_clip_record(self.G, grad_scale, self.clip_grad, self.clip_ws, self.clip_rec, self.clip_skipped)
            clip = dict(scale_rec=self.clip_rec)                 # the record carries grad_scale
        else:
            clip = dict(grad_scale=grad_scale)
        for g, wd in (("w", self.weight_decay), ("bnw", 0.0), ("bias", 0.0)):
            lo, hi = self.group[g]
            if hi <= lo:
                continue
            glr = lrs[g] if lrs is not None and g in lrs else lr
            mirror = self.P16 if g == "w" else None
            if self.optimizer == "sgd":
                sgd_step(self.P[lo:hi], self.G[lo:hi], self.Mo[lo:hi], glr, mom, wd, t == 1, mirror=mirror, **clip)
            else:
                if self.optimizer == "adamw" and self.V is None:
                    self.V = torch.zeros_like(self.P)
                optim_step(OPT_ADAMW if self.optimizer == "adamw" else OPT_SGD_NESTEROV, self.P[lo:hi], self.G[lo:hi],
                           self.Mo[lo:hi], self.V[lo:hi] if self.V is not None else None, glr, t, beta1=mom, weight_decay=wd,
                           mirror=mirror, **clip)
        if self.use_ema:
            self.ema_updates += 1
            d = self.ema_decay * (1.0 - math.exp(-self.ema_updates / self.ema_tau))
            ema_update(self.P_ema, self.P, d)
            ema_update(self.RS_ema, self.RS, d)
