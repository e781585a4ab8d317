"""Exact-integer cases, operand builders and references of the MXFP8 forward kernels: yv_linear_mxfp8 / _ex / _q on
gemm_mx_kernel (128 x 128 tiles) and gemm_p9_kernel<.., MX> (160 / 192 / 224 / 256 rows, f32-output and trainer-epilogue
instances), yv_conv2d_mxfp8 on its two tile instances.  test_mx_exact_cpu.py proves the gate without a device (preconditions,
routes, planted faults), test_gpu_mx_exact.py runs it.

Operands.  Integers of at most two significant bits (randint(-2, 3)) times a power of two per 32-element block, the exponent
taken from a pattern that differs between neighbours in every direction a kernel indexes:
    linear   A[m, k] * 2^((m + k // 32) % 4)               W[n, k] * 2^((n + k // 32) % 4)
    map i    x[b, y, x, c] * 2^((y + 2 x + 3 (c // 32) + i) % 4)   conv weight  w[co, k] * 2^((co + k // 32) % 4)
(rows m and m + 1, weight rows n and n + 1, pixels next to each other in y and in x, and the four blocks of a 128-deep K step all
carry different exponents.  The patterns first proposed for this gate, (m + 2 kb) % 4 and (3 n + kb) % 3, do not: the second does
not depend on n at all and the first repeats inside a K step, so a weight scale taken from row n + 1 or a scale byte taken from
block kb + 2 would have passed.  test_mx_exact_cpu.py asks that each such fault changes nearly every output, not one.)
Such a block survives the MXFP8 rule (mx_reference.emulate_quant) bit for bit - the builders assert it - so the device
quantisers (byte-exact by the tests of test_gpu_fp8.py / test_gpu_conv_mx.py) hand the kernels exactly these numbers, with
four distinct E8M0 scales next to each other.  Every case also carries an all-zero block (scale byte 0), a block whose only
non-zero is one element, and a block holding 7 * 2^p (448, the format maximum, after scaling).  All values are integers and
sum |a| |w| + |bias| + |res| < 2^24 (asserted), so every f32 partial sum is exact in any order: the fp32 CPU reference is THE
result, and the comparisons are torch.equal.  The one thing taken on trust is that the block-scaled MFMA sums these products
exactly; test_gpu_mx_train.py::test_wgrad_mxfp8_exact rests on the same.

Convolution inputs carry the loud borders of test_gpu_conv_routes.py::make_data (first row / column +2, last row / column -2,
times the block's power of two, in every channel of the buffer, read or not).  Outputs are prefilled with a sentinel no result
equals (0.5; bytes 0xAB, scale bytes 0xCD) and get extra rows and channels that must keep it.

Rounding rule of the bf16 shortcut of yv_conv2d_mxfp8 (csrc/gemm.hip): cgemm_mx_kernel ends in finish_tile, whose tile shapes
(NF == 4, MF even: both instances) take epilogue_staged whenever the output, the shortcut and their strides are 16-byte aligned
and "staged_epilogue" is 1 (the shipped value; every case here is aligned), and in epilogue_conv_mx when an MX map is written.
Both round the activation to bf16 in the slab BEFORE add_bf16x8 adds the shortcut: out = bf16(bf16(y) + r), two roundings - the
`staged` rule of test_gpu_conv_routes.py::expected.

Forms with a transcendental.  The argument is made exact and small by scaling weights and bias by 2^-shift (an exponent shift:
the bytes stay, the E8M0 scales move).  Every element is compared with the fp64 function of the exact argument; the bound is
half a bf16 step of the reference (one rounding of the f32 value) plus E = 2 * C, C being the largest |f32 emulation of the
expression in the kernel's source - fp64 function| over the argument range of the cases, doubled for the hardware exp2 / rcp
and for a compiler that fuses a multiply and an add the emulation rounds apart (csrc/Makefile builds with -ffp-contract=off):
    gelu_f      (csrc/gemm_common.h: x * rcp(1 + exp2(x * q(x^2))), sigmoid fit of the erf form)   C = 2.55e-05 on [-32, 32]
    gelu_grad_f (csrc/gemm_common.h: Abramowitz-Stegun 7.1.26 erfc)                                C = 2.38e-07 on [-8, 8]
    silu_f      (csrc/gemm.hip: x * rcp(1 + exp(-x)))                                              C = 1.27e-06 on [-32, 32]
(measured by form_errors() on the CPU: every multiple of 2^-10 of the range, for gelu_grad_f every bf16 value of it; recorded in
FORM_ERR and profiles/mx_exact_bounds.txt, re-measured by test_mx_exact_cpu.py).  Nothing is fitted to a kernel's output.
gelu_grad_f(0) is exactly 0.5 in that emulation, so the aux = 0 column of the GELU_BWD cases must equal bf16(bf16(lin) * 0.5)."""
import contextlib
import math

import torch
import torch.nn.functional as F

from mx_reference import dequant, emulate_quant_rows

SENTINEL, SENT_Q, SENT_S = 0.5, 0xAB, 0xCD
EXTRA_ROWS = 3
SHIPPED = {"linear_variant": 1, "linear_p8": 3, "linear_p8_rows": 0, "linear_p8_cus": 0, "staged_epilogue": 1}

# largest |f32 form - fp64 function| over the range (form_errors(); see the module docstring), and the ranges
FORM_ERR = {"gelu": 2.55e-05, "gelu_grad": 2.38e-07, "silu": 1.27e-06}
FORM_RANGE = {"gelu": 32.0, "gelu_grad": 8.0, "silu": 32.0}
AUX_ZERO_COL = 5                      # the aux = 0 column of the GELU_BWD cases


def bf(t):
    return t.to(torch.bfloat16)


@contextlib.contextmanager
def options(yv, **kw):
    """The shipped options, overridden by kw; the previous values come back afterwards."""
    want = dict(SHIPPED, **kw)
    old = {k: yv.get_option(k) for k in want}
    try:
        for k, v in want.items():
            yv.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def act_shift(kreal: int) -> int:
    """Weights and bias times 2^-shift bring the pre-activation (standard deviation ~ sqrt(595 * kreal) by the operands'
    variances) to a standard deviation of about two."""
    return max(0, int(round(0.5 * math.log2(595.0 * kreal))) - 1)


def assert_survives_quant(t: torch.Tensor, what: str):
    """Builder precondition (a): the MXFP8 rule returns t (.., C) unchanged, with at least four distinct scales."""
    q, s = emulate_quant_rows(t)
    assert torch.equal(dequant(q, s).float(), t), what
    assert len(s.unique()) >= 4, (what, s.unique().tolist())
    return q, s


def plant_blocks(ints: torch.Tensor, c0: int, c1: int):
    """ints (rows, C) integer parts (before the block's power of two): rows 1 / middle / last-but-one get, inside columns
    [c0, c1), an all-zero block, a block whose only non-zero is one element and a block holding 7."""
    rows = ints.shape[0]
    nb = (c1 - c0) // 32
    r0, r1, r2 = min(1, rows - 1), rows // 2, max(rows - 2, 0)
    b1, b2 = c0 + 32 * (nb - 1), c0 + 32 * (nb // 2)
    ints[r0, c0:c0 + 32] = 0
    ints[r1, b1:b1 + 32] = 0
    ints[r1, b1 + 19] = -1
    ints[r2, b2 + 13] = 7
    return [(r0, c0), (r1, b1), (r2, b2)]


def assert_planted(t: torch.Tensor, where):
    (r0, c0), (r1, c1), (r2, c2) = where
    assert not bool(t[r0, c0:c0 + 32].any()) and int((t[r1, c1:c1 + 32] != 0).sum()) == 1
    blk = t[r2, c2:c2 + 32].abs()
    assert float(blk.max()) == float(blk[13]) and math.log2(float(blk[13]) / 7.0).is_integer()


# ---------------------------------------------------------------------------------------------------------------- linears
LIN_SHAPES = {                       # M, N, K
    "s197": (197, 136, 128),         # one K step; M, N no multiples of 128 (N % 8 is what the API asks)
    "s300": (300, 384, 256),         # two K steps, ragged M, N % 128 == 0 (yv_linear_mxfp8_q)
    "p256": (2048 + 37, 3584, 256),  # persistent: 14 x 14 = 196 tiles of 160 rows, two K steps
    "p384": (2048 + 37, 3584, 384),  # ... an odd step count: 160 / 192 rows move to 224, f32 outputs to gemm_mx_kernel
}
M_DEV = {"s197": (3, 50), "s300": (3, 77), "p256": (3, 600), "p384": (3, 600)}      # (count, m_mul): the cut inside a tile
FAMILIES = ("plain", "f32", "pre", "gbwd")


def family_queries(yv, fam, N):
    """What a case of this epilogue family launches, as yv_linear_route takes it: (form, flags, kwargs)."""
    B, G, R, O = yv.EPI_BIAS, yv.EPI_GELU, yv.EPI_RES_F32, yv.EPI_OUT_F32
    return {"plain": [("bias", B, {}), ("gelu", B | G, {}), ("m_dev", B, dict(m_dev=True))],
            "f32": [("f32", B | O, {}), ("rmw", B | R, {}), ("res_src", B | R, dict(res_f32=True))],
            "pre": [("save_pre", B | G | yv.EPI_SAVE_PRE, dict(ldaux=N + 8))],
            "gbwd": [("gelu_bwd", B | yv.EPI_GELU_BWD, dict(ldaux=N + 8))]}[fam]


def lin_case(shape, fam, rows, kernel, tile_rows, f32out=0, ext=0):
    return dict(name=f"{shape}_{fam}_rows{rows}", shape=shape, fam=fam, rows=rows, expect=(kernel, tile_rows, f32out, ext))


def lin_cases(yv):
    """Every case names its route: (kernel, tile_rows, f32out, ext) of yv_linear_route(mx=1) under the shipped options with
    "linear_p8_rows" = rows (0: the launcher's choice)."""
    MX, P9 = yv.LIN_MX, yv.LIN_P9
    cs = [lin_case("s197", f, 0, MX, 128) for f in FAMILIES]
    cs += [lin_case("s300", "plain", 0, MX, 128), lin_case("s300", "f32", 0, MX, 128)]
    cs += [lin_case("p384", "f32", 0, MX, 128)]                   # f32 output, odd K / 128, at a persistent shape
    cs += [lin_case("p256", "plain", r, P9, r if r else 160) for r in (0, 192, 224, 256)]
    cs += [lin_case("p384", "plain", 160, P9, 224)]               # odd step count: a forced 160 runs 224
    cs += [lin_case("p256", "f32", r, P9, r if r else 160, f32out=1) for r in (0, 192, 224, 256)]
    for fam, ext in (("pre", 1), ("gbwd", 2)):
        cs += [lin_case("p256", fam, r, P9, r if r else 160, ext=ext) for r in (0, 192, 224)]
        cs += [lin_case("p384", fam, 0, P9, 224, ext=ext)]
    return cs


def lin_route(yv, c, flags, n_cu=256, **kw):
    M, N, K = LIN_SHAPES[c["shape"]]
    r = yv.linear_route(M, N, K, flags, ldo=N + 8, mx=True, n_cu=n_cu, **kw)
    assert r.mx == 1 and r.splitk == 1, r
    return (r.kernel, r.tile_rows, r.f32out, r.ext)


_LIN = {}


def lin_data(shape: str):
    """Operands and exact references of a linear shape (CPU, cached, never modified by a test): a, w, bias (f32 integers),
    lin = a w^T + bias, x (f32 residual, integers), u (bf16-representable aux of GELU_BWD with one zero column), shift."""
    if shape in _LIN:
        return _LIN[shape]
    M, N, K = LIN_SHAPES[shape]
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    kb = torch.arange(K) // 32
    ai = torch.randint(-2, 3, (M, K), generator=g).float()
    wi = torch.randint(-2, 3, (N, K), generator=g).float()
    pa, pw = plant_blocks(ai, 0, K), plant_blocks(wi, 0, K)
    a = ai * 2.0 ** ((torch.arange(M)[:, None] + kb[None]) % 4).float()
    w = wi * 2.0 ** ((torch.arange(N)[:, None] + kb[None]) % 4).float()
    assert_planted(a, pa); assert_planted(w, pw)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    x = torch.randint(-64, 65, (M, N), generator=g).float()
    u = bf((torch.randn(M, N, generator=g) * 2).clamp(-FORM_RANGE["gelu_grad"], FORM_RANGE["gelu_grad"])).float()
    u[:, AUX_ZERO_COL] = 0
    assert_survives_quant(a, shape + " A"); assert_survives_quant(w, shape + " W")
    mag = float((a.abs() @ w.abs().t()).max()) + 8 + 64
    assert mag < 2 ** 24, (shape, mag)                             # precondition (b): every partial sum is exact
    lin = a @ w.t() + bias
    shift = act_shift(K)
    assert float(lin.abs().max()) * 2.0 ** -shift <= FORM_RANGE["gelu"], shape
    _LIN[shape] = dict(M=M, N=N, K=K, a=a, w=w, bias=bias, lin=lin, x=x, u=u, shift=shift, mag=mag)
    return _LIN[shape]


# faults of the scale addressing change (nearly) every output; the others the part of the output FAULT_EXTENT names
LIN_FAULTS = ("k_block", "row", "swap_a", "w_k_block", "w_row", "swap_w", "drop_last", "stale")
SCALE_FAULTS = ("k_block", "row", "pixel", "swap_a", "w_k_block", "w_row", "swap_w")


def swap_in_step(s):
    """Scale bytes (.., blocks): block kb takes the scale of block kb ^ 2 (bytes 0 <-> 2 and 1 <-> 3 of a K step's dword: a wrong
    opsel / byte select), where that block exists."""
    nb = s.shape[-1]
    idx = torch.arange(nb) ^ 2
    idx = torch.where(idx < nb, idx, torch.arange(nb))
    return s[..., idx]


def lin_emulate(d, fault=None):
    """a w^T + bias from the quantised bytes and scales, in plain torch; `fault` plants an addressing error."""
    qa, sa = emulate_quant_rows(d["a"])
    qw, sw = emulate_quant_rows(d["w"])
    if fault == "k_block":
        sa = sa.roll(-1, 1)                                       # the scale of the neighbouring K block
    if fault == "row":
        sa = sa.roll(-1, 0)                                       # scale row m + 1
    if fault == "swap_a":
        sa = swap_in_step(sa)
    if fault == "w_k_block":
        sw = sw.roll(-1, 1)
    if fault == "w_row":
        sw = sw.roll(-1, 0)                                       # weight scale row n + 1
    if fault == "swap_w":
        sw = swap_in_step(sw)
    ad, wd = dequant(qa, sa).float(), dequant(qw, sw).float()
    if fault == "drop_last":
        ad[:, -32:] = 0                                           # the last K block dropped
    out = ad @ wd.t() + d["bias"]
    if fault == "stale":
        out[-1] = out[-2]                                         # a row of the ragged last tile left stale
    return out


# ----------------------------------------------------------------------------------------------------------- convolutions
def conv_case(name, inst, B, H, W, k, s, srcs, cout, out=(0, None), res=(0, None)):
    """srcs: [(channels, upsample, channel offset, pixel stride or 0 = dense)]; out / res: (channel offset, pixel stride or
    None = cout + 32); inst: what yv_conv2d_mxfp8_instance answers."""
    srcs = [(c, up, off, ld if ld else c) for c, up, off, ld in srcs]
    return dict(name=name, inst=inst, B=B, H=H, W=W, k=k, s=s, srcs=srcs, cout=cout, out=(out[0], out[1] or cout + 32),
                res=(res[0], res[1] or cout + 32), cin=sum(c for c, _, _, _ in srcs))


def conv_cases():
    return [
        # ---- cgemm_mx_kernel<64, 4, 1>
        conv_case("t64_3x3_kpad", 0, 2, 9, 11, 3, 1, [(96, 0, 0, 0)], 96),                        # K = 864 -> 896; 198 pixels
        conv_case("t64_3x3_s2_slice", 0, 2, 9, 8, 3, 2, [(128, 0, 32, 192)], 64, out=(8, 104), res=(16, 96)),
        conv_case("t64_1x1_two_src_96", 0, 2, 7, 10, 1, 1, [(96, 0, 0, 0), (160, 0, 32, 224)], 96),
        conv_case("t64_1x1_up_160", 0, 2, 6, 12, 1, 1, [(160, 1, 0, 0), (96, 0, 0, 0)], 32, out=(8, 48)),
        conv_case("t64_2x2_image", 0, 3, 2, 2, 3, 1, [(64, 0, 0, 0)], 64),
        conv_case("t64_1x1_s2", 0, 2, 7, 10, 1, 2, [(128, 0, 0, 0)], 160),
        # ---- cgemm_mx_kernel<128, 2, 2>: >= 100,000 output pixels and more than 64 output channels
        conv_case("t128_3x3_slice", 1, 1, 317, 320, 3, 1, [(32, 0, 32, 96)], 96, out=(8, 112), res=(8, 104)),
        conv_case("t128_3x3_s2", 1, 4, 159, 160, 3, 2, [(64, 0, 0, 0)], 96),
        conv_case("t128_1x1_two_src_96", 1, 1, 317, 320, 1, 1, [(96, 0, 0, 0), (32, 0, 0, 0)], 96),
        conv_case("t128_1x1_up_32", 1, 1, 318, 320, 1, 1, [(32, 1, 0, 0), (64, 0, 32, 96)], 160),
        conv_case("t128_2x2_images", 1, 25001, 2, 2, 3, 1, [(64, 0, 0, 0)], 96),
    ]


def conv_instance(yv, c):
    return yv.conv2d_mxfp8_instance(c["B"], c["H"], c["W"], c["k"], c["s"], c["cin"], c["cout"])


def conv_data(c):
    """Integer operands of a case (CPU) and the exact fp32 reference conv + bias, NHWC (B, H, W, cout)."""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])))
    B, H, W, k, s, cout, cin = c["B"], c["H"], c["W"], c["k"], c["s"], c["cout"], c["cin"]
    bufs, parts = [], []
    for i, (ch, up, off, ld) in enumerate(c["srcs"]):
        h, w = (H * s) >> up, (W * s) >> up
        xi = torch.randint(-2, 3, (B, h, w, ld), generator=g).float()
        xi[:, 0] = 2; xi[:, :, 0] = 2; xi[:, -1] = -2; xi[:, :, -1] = -2        # loud borders, every channel of the buffer
        where = plant_blocks(xi.view(-1, ld), off, off + ch)
        e = (torch.arange(h)[:, None, None] + 2 * torch.arange(w)[None, :, None] + 3 * (torch.arange(ld) // 32)[None, None] + i) % 4
        x = xi * 2.0 ** e.float()
        assert_planted(x.view(-1, ld), where)
        assert_survives_quant(x, f"{c['name']} source {i}")
        bufs.append(x)
        v = x[..., off:off + ch]
        if up:
            v = v.repeat_interleave(2, 1).repeat_interleave(2, 2)
        parts.append(v)
    kreal = k * k * cin
    wi = torch.randint(-2, 3, (cout, kreal), generator=g).float()              # K order (ky, kx, cin)
    where = plant_blocks(wi, 0, kreal)
    wk = wi * 2.0 ** ((torch.arange(cout)[:, None] + (torch.arange(kreal) // 32)[None]) % 4).float()
    assert_planted(wk, where)
    assert_survives_quant(pad_k128(wk), c["name"] + " weight")
    bias = torch.randint(-8, 9, (cout,), generator=g).float()
    xin = torch.cat(parts, -1).permute(0, 3, 1, 2).contiguous()
    w4 = wk.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()
    mag = float(F.conv2d(xin.abs(), w4.abs(), None, stride=s, padding=k // 2).max()) + 8 + 64
    assert mag < 2 ** 24, (c["name"], mag)                                      # precondition (b)
    ref = (F.conv2d(xin, w4, None, stride=s, padding=k // 2).permute(0, 2, 3, 1) + bias).contiguous()
    assert ref.shape == (B, H, W, cout)
    r = torch.randint(-64, 65, (B, H, W, c["res"][1]), generator=g).float()
    shift = act_shift(kreal)
    assert float(ref.abs().max()) * 2.0 ** -shift <= FORM_RANGE["silu"], c["name"]
    return dict(bufs=bufs, w=wk, bias=bias, ref=ref, res=r, shift=shift, kreal=kreal)


def pad_k128(w):
    kp = (w.shape[1] + 127) // 128 * 128
    return w if kp == w.shape[1] else torch.cat([w, w.new_zeros(w.shape[0], kp - w.shape[1])], 1)


def conv_expected(c, d, kind):
    """f32: the sum; bf16: one rounding; res: bf16(bf16(y) + r), the staged rule (module docstring)."""
    ref = d["ref"]
    if kind == "f32":
        return ref
    if kind == "bf16":
        return bf(ref)
    r = d["res"][..., c["res"][0]:c["res"][0] + c["cout"]]
    return bf(bf(ref).float() + r)


CONV_FAULTS = ("k_block", "pixel", "swap_a", "w_k_block", "w_row", "swap_w", "drop_last", "swap", "padding", "kpad_tail", "stale")


def conv_fault_applies(c, fault):
    kreal = c["k"] * c["k"] * c["cin"]
    return {"swap": len(c["srcs"]) == 2, "padding": c["k"] == 3, "kpad_tail": kreal % 128 != 0,
            "swap_a": any((cb ^ 2) < ld // 32 for ch, _, off, ld in c["srcs"] for cb in range(off // 32, (off + ch) // 32)),
            }.get(fault, True)                                     # (swap_a: a block it reads has a block kb ^ 2 in the buffer)


def conv_emulate(c, d, fault=None):
    """conv + bias from the quantised bytes and scales, in plain torch; `fault` plants an addressing error."""
    k, s, cout, cin, kreal = c["k"], c["s"], c["cout"], c["cin"], d["kreal"]
    parts = []
    for x, (ch, up, off, ld) in zip(d["bufs"], c["srcs"]):
        q, sc = emulate_quant_rows(x)
        if fault == "k_block":
            sc = sc.roll(-1, 3)                                    # the scale of the neighbouring 32-channel block
        if fault == "pixel":
            sc = sc.roll(-1, 2)                                    # the scale of the neighbouring pixel
        if fault == "swap_a":
            sc = swap_in_step(sc)
        v = dequant(q, sc).float()[..., off:off + ch]
        if up:
            v = v.repeat_interleave(2, 1).repeat_interleave(2, 2)
        parts.append(v)
    if fault == "swap":
        parts = parts[::-1]                                        # the two sources swapped
    xin = torch.cat(parts, -1).permute(0, 3, 1, 2).contiguous()
    wq, ws = emulate_quant_rows(pad_k128(d["w"]))
    if fault == "w_row":
        ws = ws.roll(-1, 0)                                        # the weight scale row n + 1
    if fault == "w_k_block":
        ws = ws.roll(-1, 1)
    if fault == "swap_w":
        ws = swap_in_step(ws)
    wd = dequant(wq, ws).float()
    tail = wd.shape[1] - kreal
    wd = wd[:, :kreal].clone()
    if fault == "drop_last":
        wd[:, -32:] = 0                                            # the last K block dropped
    pad = k // 2
    if fault == "padding":
        xin, pad = F.pad(xin, (1, 1, 1, 1), mode="replicate"), 0   # padding replaced by the neighbouring pixel
    out = F.conv2d(xin, wd.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous(), None, stride=s, padding=pad)
    out = out.permute(0, 2, 3, 1) + d["bias"]
    if fault == "kpad_tail":                                       # Kpad tail not zero: weights 1 on the pixel's first channels
        out = out + torch.cat(parts, -1)[:, ::s, ::s, :tail].sum(-1, keepdim=True)
    if fault == "stale":
        flat = out.reshape(-1, cout).clone()
        flat[-1] = flat[-2]                                        # a row of the ragged last tile left stale
        out = flat.view(out.shape)
    return out.contiguous()


# ------------------------------------------------------------------------------------------------- activation forms, bounds
def _c(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


_L2E = -1.4426950408889634


def _exp2(x):
    """exp2 of an f32 tensor, correctly rounded (through f64: the same on every host)."""
    return torch.exp2(x.double()).float()


def _rcp(x):
    return (1.0 / x.double()).float()


def gelu_form(x):
    """gelu_f of csrc/gemm_common.h, operation by operation in f32 (exp2 and the reciprocal correctly rounded)."""
    x2 = torch.minimum(x * x, _c(64.0))
    q = _fma(_c(-7.03039117e-4) * _c(_L2E), x2, _c(7.40113286e-2) * _c(_L2E))
    q = _fma(q, x2, _c(1.59501573) * _c(_L2E))
    return x * _rcp(1.0 + _exp2(x * q))


def gelu_grad_form(x):
    """gelu_grad_f of csrc/gemm_common.h in f32."""
    t = _rcp(_fma(_c(0.3275911) * _c(0.70710678118654752), x.abs(), _c(1.0)))
    p = _fma(_c(0.5) * _c(1.061405429), t, _c(0.5) * _c(-1.453152027))
    p = _fma(p, t, _c(0.5) * _c(1.421413741))
    p = _fma(p, t, _c(0.5) * _c(-0.284496736))
    p = _fma(p, t, _c(0.5) * _c(0.254829592))
    e = _exp2(x * x * _c(-0.72134752044448170368))
    w = p * t * e
    cdf = torch.where(x >= 0, 1.0 - w, w)
    return cdf + x * e * _c(0.39894228040143267794)


def silu_form(x):
    """silu_f of csrc/gemm.hip in f32: x * rcp(1 + exp(-x)), the exponential as exp2(-x * log2 e)."""
    return x * _rcp(1.0 + _exp2(x * _c(_L2E)))


def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def silu64(x):
    return x * torch.sigmoid(x)


def form_errors():
    """Largest |f32 form - fp64 function| over the ranges of FORM_RANGE: every multiple of 2^-10 (the cases' arguments are
    multiples of 2^-shift, shift <= 10), every bf16 value for gelu_grad (its argument is a bf16 tensor)."""
    out = {}
    for name, form, fn in (("gelu", gelu_form, gelu64), ("silu", silu_form, silu64)):
        R = FORM_RANGE[name]
        x = torch.arange(-int(R * 1024), int(R * 1024) + 1, dtype=torch.float64) / 1024
        out[name] = float((form(x.float()).double() - fn(x)).abs().max())
    allbf = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    x = allbf[allbf.abs() <= FORM_RANGE["gelu_grad"]]              # (NaN compares false)
    out["gelu_grad"] = float((gelu_grad_form(x).double() - gelu_grad64(x.double())).abs().max())
    return out


def half_ulp_bf16(v):
    """Half the spacing of bf16 (8 significant bits) in the binade of |v|: 2^(floor(log2 |v|) - 8)."""
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** -120))           # |v| = m * 2^ex, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), ex - 9)


def act_bound(ref, err):
    """One bf16 rounding of a value within `err` (tensor or number) of the fp64 reference."""
    return half_ulp_bf16(ref.abs() + err) + err


def first_diff(got, exp):
    bad = (got.float() != exp.float()).nonzero()
    i = tuple(bad[0].tolist())
    return f"{len(bad)} of {got.numel()} values differ, first at {i}: got {float(got[i])}, expected {float(exp[i])}"
