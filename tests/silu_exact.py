"""Exact cases and float64 references of the two detector kernels that have SiLU BETWEEN their layers: yv_c2f_fused
(csrc/c2f.hip) and the matrix-pipe stem (stem_mfma_kernel, csrc/yolo_misc.hip).  test_silu_exact_cpu.py proves the gate without a
device (conditions, order independence, planted faults), test_gpu_silu_exact.py runs it.

The regime.  All three kernels write SiLU as x * rcp(1.0f + __expf(-x)).  For x >= 17, exp(-x) is below half an f32 step at 1.0,
so 1 + exp(-x) is exactly 1.0f and the expression returns x bit for bit (IDENTITY_FROM; the cases keep every pre-activation at
FLOOR = 24 or above, the device premise is checked first by test_gpu_silu_exact.py).  With operands that are bf16 values, weights
that are small integers times a power of two and every partial sum below 2^24 steps of the finest term, the f32 accumulation is
exact in ANY order, the only rounding of a layer is the round-to-nearest-even of its output to bf16, and a float64 reference
reproduces the whole chain of 4 or 6 layers bit for bit: the comparisons are torch.equal.  Pixels outside the image are ZERO in
every intermediate (the rule of c2f.hip); here a pixel that should be 0 would otherwise be >= 24.

What the regime cannot see: the SiLU curve itself and negative values.  Those stay with test_gpu_conv_routes.py::
test_silu_epilogues_by_element (same expression on the layer kernels) and the tolerance tests of the two kernels, which remain.

Operands.
    C2f   x: integers in [16, 32]; weights: integers in [-2, 2] times 2^-s, s = 2 (cv1), 5 (3 x 3 layers), 4 (cv2); bias per
          channel ceil(FLOOR - min over the case's pixels of the exact sum) - the bias is an INPUT of the case, computed layer by
          layer over both rounding rules of the shortcut (below) so that either chain stays at or above FLOOR.
    stem  pixels: random uint8; weights from {0, +-255/2, +-255/4, +-255/8, +-255/16}: the kernel forms w * (1.0f / 255.0f) in
          f32 and splits it into a bf16 high and low half; 255 * fl(1/255) rounds to exactly 1.0f, so these (and, of 255 * m,
          only m = 0 and +-2^i) give the exact dyadic +-2^-j with a zero low half - asserted in numpy float32 by the builder.
Loud borders as in test_gpu_conv_routes.py::make_data: first row / column at the top of the range, last row / column at the
bottom, in every channel of the buffer whether read or not.  (Stem: 255 and 64, not 0 - 0 is what the padding itself reads, and
a left padding taken from the previous row's end would go unseen.)

The two rounding rules of the shortcut.  c2f.hip adds the bottleneck's input in f32 and rounds once, bf16(pre + y), as the layer
kernels' direct epilogue does; their staged epilogue rounds first, bf16(bf16(pre) + y) (test_gpu_conv_routes.py::
test_shortcut_rounding_rule).  c2f_reference states either; every case with a shortcut must tell them apart (condition d).

Conditions, asserted by the builders for every case they return (ConditionError otherwise):
    (a) every pre-activation of every layer >= FLOOR;
    (b) per layer (max over outputs of sum |w| |x|, + max |b|, + max |shortcut|) / (smallest step of any term) < 2^24;
    (c) every nonzero intermediate >= 16: its bf16 step is >= 2^-3, the granularity (b) uses;
    (d) with a shortcut, the two rounding rules differ on at least one output element."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 0.5
FLOOR = 24.0                # the smallest pre-activation of any case
IDENTITY_FROM = 17.0        # x * rcp(1.0f + expf(-x)) == x in f32 from here on (exp(-17) = 4.1e-8 < 2^-24: see _check_identity)
TILE = 16                   # c2f_fused_kernel's output tile

C2F_INSTANCES = [(16, 1), (16, 2), (32, 1), (32, 2)]
C2F_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 16, 16), (1, 17, 16), (1, 16, 33), (2, 21, 37)]
C2F_STRIDED_SHAPE = (2, 21, 37)
STEM_COUTS = (16, 32, 48)
STEM_SHAPES = [(1, 2, 128), (2, 4, 256), (1, 6, 384)]
STEM_GRID_STRIDE = (4, 4100, 128, 16)                    # 8200 chunks of 64 output pixels against 2048 x 4 grid slots
STEM_GRID_SLOTS = 2048 * 4
STEM_WEIGHTS = (0.0, 127.5, -127.5, 63.75, -63.75, 31.875, -31.875, 15.9375, -15.9375)


class ConditionError(AssertionError):
    pass


def _need(ok, *what):
    if not ok:
        raise ConditionError(*what)


def _check_identity():
    """The arithmetic of the regime in IEEE float32: 1 + exp(-x) == 1 from IDENTITY_FROM on."""
    for v in (IDENTITY_FROM, 20.0, FLOOR):
        assert np.float32(1.0) + np.exp(np.float32(-v)) == np.float32(1.0), v
    assert np.float32(1.0) + np.exp(np.float32(-16.0)) != np.float32(1.0)


_check_identity()


def bf16_round(v):
    """Round-to-nearest-even to 8 significant bits in float64 (the cases stay far from bf16's exponent limits): written out, not
    borrowed from torch's bf16 cast - test_silu_exact_cpu.py checks the two against each other."""
    m, e = torch.frexp(v)                                 # v = m * 2^e, |m| in [0.5, 1)
    return torch.ldexp(torch.round(m * 256.0), e - 8)    # torch.round: halves to even


def silu64(v):
    """SiLU as the regime has it: the identity from IDENTITY_FROM on; the real function below (reached only by the planted fault
    that leaves out-of-image intermediates at their computed value)."""
    return torch.where(v >= IDENTITY_FROM, v, v * torch.sigmoid(v))


def conv64(x, w, k, stride=1, padding=None):
    """x (B, C, H, W) float64, w (Cout, k * k * C) in the K order (ky, kx, c) the kernels take -> exact sums."""
    co, c = w.shape[0], x.shape[1]
    w4 = w.double().reshape(co, k, k, c).permute(0, 3, 1, 2).contiguous()
    return F.conv2d(x, w4, None, stride=stride, padding=k // 2 if padding is None else padding)


def c2f_layer_names(n):
    return ["cv1"] + [f"m{j}.cv{i}" for j in range(n) for i in (1, 2)] + ["cv2"]


def c2f_chain(x, weights, biases, c, n, staged=False, shortcut_from=None, cv2_order=None, pad=0, masked=True, upto=None):
    """The block on float64: x (B, H, W, 2c) -> (out (B, H, W, 2c), layers).  States the rule of c2f.hip:
        y0 | y1 = bf16(cv1 x + b)                                     1 x 1
        t_j     = bf16(m_j.cv1 * y(j+1) + b)                          3 x 3, zero outside the image
        y(j+2)  = bf16(m_j.cv2 * t_j + b + y(j+1))                    3 x 3, ONE rounding (staged: bf16(bf16(..) + y(j+1)))
        out     = bf16(cv2 [y0 | y1 | .. | y(n+1)] + b)               1 x 1
    with SiLU the identity (every pre-activation >= FLOOR: build_c2f asserts it on `layers`).  K order does not matter: the sums
    are exact.  layers: per layer dict(name, inp, w, k, sum, pre, res) for the conditions; `upto` stops after that many layers.
    The keyword arguments plant faults (test_silu_exact_cpu.py): shortcut_from(j) = index of the array the shortcut of bottleneck
    j is read from (the rule: j + 1), cv2_order = order of cv2's sources, pad > 0 with masked = False = the block computed on an
    image zero-extended by `pad` pixels whose out-of-image intermediates keep their computed value."""
    B, H, W, _ = x.shape
    xin = x.double().permute(0, 3, 1, 2)
    if pad:
        xin = F.pad(xin, (pad, pad, pad, pad))
    inimg = torch.zeros(1, 1, H + 2 * pad, W + 2 * pad, dtype=torch.float64)
    inimg[..., pad:pad + H, pad:pad + W] = 1.0
    keep = (lambda v: v * inimg) if masked else (lambda v: v)
    layers = []

    def layer(name, inp, k, res=None):
        i = len(layers)
        s = conv64(inp, weights[i], k)
        pre = s + biases[i].double().view(1, -1, 1, 1)
        layers.append(dict(name=name, inp=inp, w=weights[i], k=k, sum=s, pre=pre, res=res))
        a = silu64(pre)
        if res is None:
            return keep(bf16_round(a))
        return keep(bf16_round(bf16_round(a) + res) if staged else bf16_round(a + res))

    def done():
        return upto is not None and len(layers) >= upto

    y = layer("cv1", xin, 1)
    ys = [y[:, :c], y[:, c:]]
    for j in range(n):
        if done():
            return None, layers
        t = layer(f"m{j}.cv1", ys[-1], 3)
        if done():
            return None, layers
        ys.append(layer(f"m{j}.cv2", t, 3, res=ys[shortcut_from(j) if shortcut_from else j + 1]))
    if done():
        return None, layers
    order = cv2_order if cv2_order is not None else range(n + 2)
    out = layer("cv2", torch.cat([ys[i] for i in order], 1), 1)
    return out[..., pad:pad + H, pad:pad + W].permute(0, 2, 3, 1).contiguous(), layers


def c2f_reference(case, staged=False, **fault):
    """The float64 result of a case under the single-rounding rule of c2f.hip (staged = False) or the layer kernels' staged one."""
    return c2f_chain(case["x"], case["w"], case["b"], case["c"], case["n"], staged=staged, **fault)[0]


def layer_bits(lay, w_shift, in_step):
    """Condition (b) of one layer: log2 of (largest sum |w| |x| + |b| + |shortcut|) / (smallest step of any term)."""
    mag = float(conv64(lay["inp"].abs(), lay["w"].abs(), lay["k"]).max()) + float((lay["pre"] - lay["sum"]).abs().max())
    if lay["res"] is not None:
        mag += float(lay["res"].abs().max())
    return math.log2(mag / (2.0 ** -w_shift * in_step))


C2F_W_SHIFT = {"cv1": 2, "m": 5, "cv2": 4}


def _c2f_shift(name):
    return C2F_W_SHIFT["m" if name.startswith("m") else name]


def check_c2f_conditions(case):
    """(a) - (d) of the module docstring for both chains of a case; returns the figures (smallest pre-activation, largest value,
    worst bit count of (b), fraction of outputs on which the two rounding rules differ)."""
    stats = dict(min_pre=math.inf, max_val=0.0, bits=0.0)
    for staged in (False, True):
        _, layers = c2f_chain(case["x"], case["w"], case["b"], case["c"], case["n"], staged=staged)
        for lay in layers:
            lo = float(lay["pre"].min())
            _need(lo >= FLOOR, "(a)", case["name"], lay["name"], staged, lo)
            nz = lay["inp"][lay["inp"] != 0]
            _need(nz.numel() == 0 or float(nz.abs().min()) >= 16, "(c)", case["name"], lay["name"], staged)
            _need(bool((bf16_round(lay["inp"]) == lay["inp"]).all()), "operands are bf16 values", case["name"], lay["name"])
            in_step = 1.0 if lay["name"] == "cv1" else 2.0 ** -3          # x: integers; intermediates: bf16 values >= 16
            bits = layer_bits(lay, _c2f_shift(lay["name"]), in_step)
            _need(bits < 24, "(b)", case["name"], lay["name"], staged, bits)
            top = float(lay["pre"].max()) + (float(lay["res"].max()) if lay["res"] is not None else 0.0)
            stats = dict(min_pre=min(stats["min_pre"], lo), max_val=max(stats["max_val"], top), bits=max(stats["bits"], bits))
    for w, name in zip(case["w"], c2f_layer_names(case["n"])):
        q = w.double() * 2.0 ** _c2f_shift(name)
        _need(bool((q == q.round()).all()) and float(q.abs().max()) <= 2, "weights", case["name"], name)
    stats["rules_differ"] = float((case["ref"] != case["ref_staged"]).double().mean())
    _need(stats["rules_differ"] > 0, "(d)", case["name"])
    return stats


def c2f_name(c, n, B, H, W, strided=False):
    return f"c{c}n{n}_{B}x{H}x{W}" + ("_strided" if strided else "")


@functools.lru_cache(maxsize=None)
def build_c2f(c, n, B, H, W, strided=False):
    """One C2f case: operands as CPU float tensors holding bf16-exact values (biases f32 integers) and both references.
    strided: x is the channel slice at offset 8 of a buffer of 2c + 8 channels, out the slice at offset 4 of one of 2c + 4 - both
    legal by the checks of yv_c2f_fused (x 16-byte aligned with a stride of a multiple of 8 elements, out 8 / 4)."""
    name = c2f_name(c, n, B, H, W, strided)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    C1 = 2 * c
    x_off, x_ld, out_off, out_ld = (8, C1 + 8, 4, C1 + 4) if strided else (0, C1, 0, C1)
    xbuf = torch.randint(16, 33, (B, H, W, x_ld), generator=g).float()
    xbuf[:, -1] = 16; xbuf[:, :, -1] = 16; xbuf[:, 0] = 32; xbuf[:, :, 0] = 32       # loud borders, every channel of the buffer
    shapes = [(C1, C1)] + [(c, 9 * c)] * (2 * n) + [(C1, (2 + n) * c)]
    names = c2f_layer_names(n)
    weights = [torch.randint(-2, 3, s, generator=g).float() * 2.0 ** -_c2f_shift(nm) for s, nm in zip(shapes, names)]
    biases = [torch.zeros(s[0]) for s in shapes]
    x = xbuf[..., x_off:x_off + C1]
    for i in range(len(shapes)):                          # the bias of layer i from the sums of layer i of BOTH chains
        lo = None
        for staged in (False, True):
            lay = c2f_chain(x, weights, biases, c, n, staged=staged, upto=i + 1)[1][i]
            m = lay["sum"].amin(dim=(0, 2, 3))
            lo = m if lo is None else torch.minimum(lo, m)
        biases[i] = torch.ceil(FLOOR - lo).float()
    case = dict(name=name, c=c, n=n, B=B, H=H, W=W, xbuf=xbuf, x_off=x_off, out_off=out_off, out_ld=out_ld, x=x, w=weights, b=biases)
    case["ref"] = c2f_reference(case)
    case["ref_staged"] = c2f_reference(case, staged=True)
    case["stats"] = check_c2f_conditions(case)
    return case


def c2f_cases():
    """(c, n, B, H, W, strided) of every C2f case of test_gpu_silu_exact.py."""
    return [(c, n, *s, False) for c, n in C2F_INSTANCES for s in C2F_SHAPES] + \
           [(c, n, *C2F_STRIDED_SHAPE, True) for c, n in C2F_INSTANCES]


def c2f_tile_reference(case, b, ty, tx, halo):
    """The 16 x 16 output tile (ty, tx) of image b computed from the part of x within `halo` pixels of the tile alone (what lies
    beyond reads as zero, as beyond the image): with halo = 2 n, the kernel's, this IS the tile of the reference."""
    H, W = case["H"], case["W"]
    y0, x0 = ty * TILE, tx * TILE
    y1, x1 = min(y0 + TILE, H), min(x0 + TILE, W)
    ya, xa, yb, xb = max(y0 - halo, 0), max(x0 - halo, 0), min(y1 + halo, H), min(x1 + halo, W)
    out = c2f_chain(case["x"][b:b + 1, ya:yb, xa:xb], case["w"], case["b"], case["c"], case["n"])[0]
    return out[0, y0 - ya:y1 - ya, x0 - xa:x1 - xa]


def seam_mask(H, W):
    """Pixels on a tile seam (first / last row or column of a 16 x 16 tile) or on the image border."""
    yy, xx = torch.arange(H).view(-1, 1), torch.arange(W).view(1, -1)
    edge = lambda v, n: (v % TILE == 0) | (v % TILE == TILE - 1) | (v == n - 1)
    return edge(yy, H) | edge(xx, W)


def describe_c2f_mismatch(case, got, want):
    """First wrong element of a (B, H, W, 2c) result as image, tile, position inside the tile (rim or interior), channel."""
    bad = (got != want).nonzero()
    b, y, x, ch = bad[0].tolist()
    py, px = y % TILE, x % TILE
    where = "rim" if bool(seam_mask(case["H"], case["W"])[y, x]) else "interior"
    return (f"{case['name']}: {len(bad)} of {want.numel()} values differ; first: image {b}, tile (ty, tx) = ({y // TILE}, {x // TILE}), "
            f"position (py, px) = ({py}, {px}) [{where}], channel {ch}: got {float(got[b, y, x, ch])}, want {float(want[b, y, x, ch])}")


# ------------------------------------------------------------------------------------------------ stem
def stem_name(B, H, W, cout, ld=None):
    return f"stem{cout}_{B}x{H}x{W}" + (f"_ld{ld}" if ld and ld != cout else "")


def stem_sum(img, w27, **kw):
    """img (B, H, W, 3) -> exact sums (B, cout, H / 2, W / 2) of the 3 x 3 / stride 2 / pad 1 convolution with w / 255;
    w27 (27, cout) in the kernel's layout, row (ky * 3 + kx) * 3 + c."""
    return conv64(img.double().permute(0, 3, 1, 2), (w27.double() / 255.0).t().contiguous(), 3, stride=2, **kw)


def stem_reference(case, img=None, **kw):
    s = stem_sum(case["img"] if img is None else img, case["w"], **kw)
    return bf16_round(s + case["b"].double().view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def build_stem(B, H, W, cout, ld=None):
    """One stem case: img (B, H, W, 3) u8, w (27, cout) f32, b (cout) f32 and the float64 reference (B, H / 2, W / 2, cout)."""
    assert W % 128 == 0 and H % 2 == 0, "the matrix-pipe form of yv_stem_conv"
    name = stem_name(B, H, W, cout, ld)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    img[:, -1] = 64; img[:, :, -1] = 64; img[:, 0] = 255; img[:, :, 0] = 255
    w = torch.tensor(STEM_WEIGHTS)[torch.randint(0, len(STEM_WEIGHTS), (27, cout), generator=g)]
    eff = w.numpy().astype(np.float32) * (np.float32(1.0) / np.float32(255.0))       # what stem_mfma_kernel forms, in f32
    want = (w.double() / 255.0).numpy()
    _need(bool((eff.astype(np.float64) == want).all()), "w * fl(1 / 255) is not the intended +-2^-j", name)
    m, _ = np.frexp(want[want != 0])
    _need(bool((np.abs(m) == 0.5).all()), "a power of two: the bf16 high half holds it, the low half is 0", name)
    case = dict(name=name, B=B, H=H, W=W, cout=cout, ld=ld or cout, img=img, w=w, b=torch.zeros(cout))
    s = stem_sum(img, w)
    case["b"] = torch.ceil(FLOOR - s.amin(dim=(0, 2, 3))).float()
    pre = s + case["b"].double().view(1, -1, 1, 1)
    _need(float(pre.min()) >= FLOOR, "(a)", name)
    mag = float(stem_sum(img, w.abs()).max()) + float(case["b"].abs().max())
    bits = math.log2(mag / 2.0 ** -4)                                                # products: integers times 2^-4 at the finest
    _need(bits < 24, "(b)", name, bits)
    case["ref"] = stem_reference(case)
    case["stats"] = dict(min_pre=float(pre.min()), max_val=float(pre.max()), bits=bits)
    return case


def stem_cases():
    """(B, H, W, cout, ld) of every stem case of test_gpu_silu_exact.py; the last but one is the grid-stride case, the last has
    out_ld > cout."""
    B, H, W, co = STEM_GRID_STRIDE
    assert B * (H // 2) * (W // 2) // 64 > STEM_GRID_SLOTS
    return [(*s, co_, None) for co_ in STEM_COUTS for s in STEM_SHAPES] + [(B, H, W, co, None), (2, 4, 256, 32, 40)]


def sum_f32_ordered(lay_inp, w, k, stride, reverse, padding=None):
    """The sum of one layer in FLOAT32, one K slot after the other in forward or reversed order (im2col by F.unfold):
    (B, Cout, L)."""
    x = lay_inp.float()
    cols = F.unfold(x, k, padding=k // 2 if padding is None else padding, stride=stride)          # (B, C * k * k, L), K order (c, ky, kx)
    co, c = w.shape[0], x.shape[1]
    wk = w.float().reshape(co, k, k, c).permute(0, 3, 1, 2).reshape(co, -1)
    acc = torch.zeros(x.shape[0], co, cols.shape[-1])
    ks = range(cols.shape[1])
    for i in (reversed(ks) if reverse else ks):
        acc = acc + wk[:, i].view(1, -1, 1) * cols[:, i:i + 1]
    return acc
