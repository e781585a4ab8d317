"""Every route of the bf16 convolution (yv_conv2d: six kernel instantiations, two epilogue forms, split-K) against an exact
integer reference.

Operands are small integers, so every product and every f32 partial sum is an integer below 2^24: the CPU reference
(F.conv2d in fp32) is exact whatever its summation order, and so is the kernel's.  A wrong tap bit, pixel offset, ring slot,
K step or edge tile is therefore a wrong integer somewhere, and the comparisons are torch.equal, not norms.  Inputs carry loud
borders (first row / column +A, last row / column -A, in every channel of the buffer, read or not) so that a tap that reads a
neighbour instead of the padding, or the previous row instead of "left of column 0", changes the sum.  Outputs are prefilled
with 0.5, which no integer result equals.

Each case names the route code (yvhip.conv2d_instance) it is there for and asserts it before running: a change of the
dispatch thresholds turns the case red instead of quietly moving it to another kernel."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0.5
SHIPPED = {"conv_dma": 8, "conv_splitk": 0, "staged_epilogue": 1}
KINDS = ("bf16", "f32", "res")


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


class Options:
    """Shipped options overridden by kw; previous values (read with get_option) restored on exit."""

    def __init__(self, yv, **kw):
        self.yv, self.want = yv, dict(SHIPPED, **kw)

    def __enter__(self):
        self.old = {k: self.yv.get_option(k) for k in self.want}
        try:
            for k, v in self.want.items():
                self.yv.set_option(k, v)
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.yv.set_option(k, v)
        return False


def bf(t):
    return t.to(torch.bfloat16)


def case(name, B, H, W, k, s, srcs, cout, expect, out=(0, None), res=(0, None), kinds=KINDS, query=None):
    """srcs: [(channels, upsample, channel offset, pixel stride)] ; out / res: (channel offset, pixel stride or None = dense);
    expect: the route that runs; query: what conv2d_instance answers where that differs (it assumes 16-byte aligned bases)."""
    srcs = [(c, up, off, ld if ld else c) for c, up, off, ld in srcs]
    return dict(name=name, B=B, H=H, W=W, k=k, s=s, srcs=srcs, cout=cout, expect=expect, out=(out[0], out[1] or cout),
                res=(res[0], res[1] or cout), kinds=kinds, query=expect if query is None else query)


def make_data(c, seed, amp=2, wamp=2, ramp=64):
    """Integer operands of a case (CPU) and the exact fp32 reference conv + bias, NHWC."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, k, s = c["B"], c["H"], c["W"], c["k"], c["s"]
    bufs, parts = [], []
    for ch, up, off, ld in c["srcs"]:
        h, w = (H * s) >> up, (W * s) >> up
        x = torch.randint(-amp, amp + 1, (B, h, w, ld), generator=g).float()
        x[:, 0] = amp; x[:, :, 0] = amp; x[:, -1] = -amp; x[:, :, -1] = -amp          # loud borders, every channel of the buffer
        bufs.append(x)
        v = x[..., off:off + ch]
        if up:
            v = v.repeat_interleave(2, 1).repeat_interleave(2, 2)
        parts.append(v)
    cin = sum(ch for ch, _, _, _ in c["srcs"])
    wk = torch.randint(-wamp, wamp + 1, (c["cout"], k, k, cin), generator=g).float()      # K order (ky, kx, cin)
    bias = torch.randint(-8, 9, (c["cout"],), generator=g).float()
    xin = torch.cat(parts, -1).permute(0, 3, 1, 2).contiguous()
    lin = F.conv2d(xin, wk.permute(0, 3, 1, 2).contiguous(), None, stride=s, padding=k // 2)
    assert k * k * cin * amp * wamp + 8 < 2 ** 24                 # every partial sum, in any order, is an exact integer
    ref = lin.permute(0, 2, 3, 1).contiguous() + bias
    assert float(ref.abs().max()) < 2 ** 24 and ref.shape == (B, H, W, c["cout"])
    r = torch.randint(-ramp, ramp + 1, (B, H, W, c["res"][1]), generator=g).float()
    return dict(bufs=bufs, w=wk.reshape(c["cout"], k * k * cin), bias=bias, ref=ref, res=r)


def to_device(c, d):
    d["bufs_d"] = [bf(x).to(DEV) for x in d["bufs"]]
    d["w_d"], d["bias_d"], d["res_d"] = bf(d["w"]).to(DEV), d["bias"].to(DEV), bf(d["res"]).to(DEV)
    return d


def expected(c, d, kind, staged):
    """The rounding rule of test_shortcut_rounding_rule: the staged epilogue rounds the activation before it adds the shortcut."""
    ref = d["ref"]
    if kind == "f32":
        return ref
    if kind == "bf16":
        return bf(ref)
    r = d["res"][..., c["res"][0]:c["res"][0] + c["cout"]]
    return bf(bf(ref).float() + r) if staged else bf(ref + r)


def kind_flags(yv, kind):
    return {"bf16": 0, "f32": yv.EPI_OUT_F32, "res": yv.EPI_RES_BF16}[kind]


def query(yv, c, flags):
    c1 = c["srcs"][1][0] if len(c["srcs"]) > 1 else 0
    return yv.conv2d_instance(c["B"], c["H"], c["W"], c["k"], c["s"], c["srcs"][0][0], c1, c["cout"], c["out"][1],
                              c["res"][1] if flags & yv.EPI_RES_BF16 else 0, flags)


def launch(yv, c, d, flags):
    """Runs the case with the epilogue `flags`; returns the whole output buffer (prefilled with the sentinel)."""
    f32 = bool(flags & yv.EPI_OUT_F32)
    out = torch.full((c["B"], c["H"], c["W"], c["out"][1]), SENTINEL, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
    views = [yv.view(t, off, ch, up) for t, (ch, up, off, _) in zip(d["bufs_d"], c["srcs"])]
    has_res = bool(flags & yv.EPI_RES_BF16)
    yv.conv2d(views[0], views[1] if len(views) > 1 else None, c["B"], c["H"], c["W"], c["k"], c["s"], d["w_d"], d["bias_d"], out,
              c["out"][0], flags, res=d["res_d"] if has_res else None, res_c_off=c["res"][0] if has_res else 0)
    torch.cuda.synchronize()
    return out


def split_out(c, out):
    off, co = c["out"][0], c["cout"]
    return out[..., off:off + co], torch.cat([out[..., :off], out[..., off + co:]], -1)


def check_exact(yv, c, d, kind, staged, what=""):
    out = launch(yv, c, d, kind_flags(yv, kind))
    got, outside = split_out(c, out)
    exp = expected(c, d, kind, staged).to(DEV)
    assert bool((outside == SENTINEL).all()), (c["name"], kind, what, "wrote outside its channels")
    if not torch.equal(got, exp):
        bad = (got.float() != exp.float()).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{c['name']} {kind} {what}: {len(bad)} of {got.numel()} values differ, first at (b, y, x, n) = {i}: "
                             f"got {float(got[i])}, expected {float(exp[i])}")


def codes(yv):
    S = yv.CONV_STAGED
    return dict(I16=yv.CONV_IGEMM_16, I32=yv.CONV_IGEMM_32, I64=yv.CONV_IGEMM_64 | S, I128=yv.CONV_IGEMM_128 | S,
                I64_DIRECT=yv.CONV_IGEMM_64, D64=yv.CONV_DMA_64_3 | S, D128=yv.CONV_DMA_128_2 | S, TWO=yv.CONV_TWO)


def cases(yv):
    k = codes(yv)
    I16, I32, I64, I128, D64, D128, TWO = k["I16"], k["I32"], k["I64"], k["I128"], k["D64"], k["D128"], k["TWO"]
    return [
        # ---- igemm_kernel: each tile width; Cin that is not tap-uniform; K = 216 not a multiple of 64
        case("igemm16", 2, 10, 12, 3, 1, [(32, 0, 0, 0)], 16, I16),
        case("igemm32_cin24", 2, 9, 11, 3, 1, [(24, 0, 0, 0)], 32, I32),
        case("igemm32_cin24_s2", 1, 7, 5, 3, 2, [(24, 0, 8, 40)], 24, I32, out=(8, 40), res=(16, 48)),
        case("igemm64_cin48", 2, 11, 9, 3, 2, [(48, 0, 0, 0)], 64, I64),
        case("igemm64_cin48_1x1", 3, 13, 13, 1, 1, [(48, 0, 16, 72)], 40, I64, out=(8, 56), res=(8, 48)),
        case("igemm128_ragged_n", 2, 17, 9, 3, 1, [(32, 0, 0, 0)], 96, I128),
        case("igemm128_cin96", 1, 13, 13, 1, 1, [(96, 0, 0, 0)], 144, I128),
        case("igemm_two_src_up_narrow", 2, 12, 10, 1, 1, [(32, 1, 0, 0), (16, 0, 0, 0)], 24, I32 | TWO),
        case("igemm_two_src_up_staged", 2, 12, 10, 1, 1, [(32, 1, 8, 48), (32, 0, 0, 0)], 64, I64 | TWO),
        case("igemm_two_src_second_up", 1, 10, 14, 1, 1, [(40, 0, 0, 0), (88, 1, 8, 96)], 136, I128 | TWO),
        # a bf16 output at channel offset 4 is 8-byte aligned: no staged epilogue, hence no LDS-DMA route (the query assumes alignment)
        case("out_c_off4_direct_epilogue", 2, 10, 10, 3, 1, [(64, 0, 0, 0)], 64, k["I64_DIRECT"], out=(4, 72), kinds=("bf16", "res"),
             query=D64),
        # ---- cgemm_dma_kernel<64,4,1,3>: K steps 1, 2, 10 (1 x 1) and 9, 18, 27, 81 (3 x 3) in a 3-stage ring
        case("dma64_1x1_nk1", 2, 13, 13, 1, 1, [(64, 0, 0, 0)], 64, D64),
        case("dma64_1x1_nk2_n80", 2, 9, 15, 1, 1, [(128, 0, 0, 0)], 80, D64),
        case("dma64_1x1_nk10_n144", 1, 12, 12, 1, 1, [(640, 0, 0, 0)], 144, D64),
        case("dma64_3x3_cin64", 2, 20, 20, 3, 1, [(64, 0, 0, 0)], 64, D64),
        case("dma64_3x3_cin128", 2, 20, 20, 3, 1, [(128, 0, 0, 0)], 128, D64),
        case("dma64_3x3_cin192_m169", 1, 13, 13, 3, 1, [(192, 0, 0, 0)], 64, D64),
        case("dma64_3x3_cin576_n192", 1, 10, 10, 3, 1, [(576, 0, 0, 0)], 192, D64),
        case("dma64_stride2", 2, 10, 9, 3, 2, [(64, 0, 0, 0)], 80, D64),
        case("dma64_stride2_1x1", 2, 8, 8, 1, 2, [(128, 0, 0, 0)], 64, D64),
        case("dma64_17x33", 1, 17, 33, 3, 1, [(128, 0, 0, 0)], 192, D64),
        case("dma64_33x17_cin192", 2, 33, 17, 3, 1, [(192, 0, 0, 0)], 144, D64),
        case("dma64_2x2_image", 1, 2, 2, 3, 1, [(64, 0, 0, 0)], 64, D64),
        case("dma64_2x2_images", 3, 2, 2, 3, 1, [(128, 0, 0, 0)], 80, D64),
        case("dma64_1x1_image", 5, 1, 1, 3, 1, [(64, 0, 0, 0)], 64, D64),
        # a channel slice of a wider buffer: the pixel "left of column 0" is real memory of the previous row
        case("dma64_slices_3x3", 2, 12, 14, 3, 1, [(64, 0, 8, 136)], 64, D64, out=(8, 88), res=(16, 96)),
        case("dma64_slices_3x3_s2", 2, 7, 9, 3, 2, [(128, 0, 64, 200)], 144, D64, out=(16, 168), res=(8, 160)),
        case("dma64_slices_1x1", 2, 13, 13, 1, 1, [(64, 0, 72, 144)], 80, D64, out=(24, 104), res=(80, 160)),
        case("dma64_two_src_128up_64", 2, 12, 10, 1, 1, [(128, 1, 0, 0), (64, 0, 0, 0)], 144, D64),
        case("dma64_two_src_64_128up", 2, 10, 12, 1, 1, [(64, 0, 0, 0), (128, 1, 0, 0)], 64, D64),
        case("dma64_two_src_128up_128", 2, 12, 10, 1, 1, [(128, 1, 0, 0), (128, 0, 0, 0)], 80, D64),
        case("dma64_two_src_slices", 1, 14, 18, 1, 1, [(64, 1, 8, 80), (64, 0, 64, 136)], 80, D64, out=(8, 96), res=(8, 88)),
        # ---- cgemm_dma_kernel<128,2,2,2>: >= 100,000 output pixels and more than 64 output channels (what bench.py runs)
        case("dma128_b16_80x80_3x3", 16, 80, 80, 3, 1, [(64, 0, 0, 0)], 128, D128),
        case("dma128_b16_80x80_two_src", 16, 80, 80, 1, 1, [(128, 1, 0, 0), (64, 0, 0, 0)], 128, D128),
        case("dma128_320x320_n80", 1, 320, 320, 1, 1, [(64, 0, 0, 0)], 80, D128),
        case("dma128_315x320_slices", 1, 315, 320, 3, 1, [(64, 0, 8, 72)], 136, D128, out=(8, 152), res=(8, 144), kinds=("res", "f32")),
    ]


def case_names():
    import yvhip
    return [c["name"] for c in cases(yvhip)]


def covered_codes(yv):
    return {c["expect"] for c in cases(yv)}


# ------------------------------------------------------------------------------------------------ B.1
@pytest.mark.parametrize("name", case_names())
def test_exact_integer_parity(yv, name):
    """bias -> bf16, bias -> f32 and bias + bf16 shortcut of every case, element for element, on the route the case names."""
    c = next(x for x in cases(yv) if x["name"] == name)
    with Options(yv):
        d = to_device(c, make_data(c, seed=sum(map(ord, name))))
        for kind in c["kinds"]:
            assert query(yv, c, kind_flags(yv, kind)) == c["query"], (name, kind)
            check_exact(yv, c, d, kind, staged=bool(c["expect"] & yv.CONV_STAGED))


def test_subbatched_source_on_the_lds_dma_route(yv):
    """A source beyond 2 GB (40 images of 320 x 320 pixels at a pixel stride of 336 channels) of which 64 channels are read: the
    host takes it in sub-batches of 31 images, each on the LDS-DMA route.  The result on the big buffer equals the result on a
    compact copy of the slice, and the first and the last image equal the CPU integer reference (3 x 3 / stride 2, and 1 x 1 with
    the bf16 shortcut read from the same slice)."""
    B, H, ld, c, co, off = 40, 320, 336, 64, 64, 8
    g = torch.Generator(device=DEV).manual_seed(5)
    big = torch.randint(-2, 3, (B, H, H, ld), generator=g, device=DEV, dtype=torch.int8).to(torch.bfloat16)
    assert big.numel() * 2 > 2 ** 31
    big[:, 0] = 2; big[:, :, 0] = 2; big[:, -1] = -2; big[:, :, -1] = -2
    small = big[..., off:off + c].contiguous()
    gc = torch.Generator().manual_seed(6)
    w3 = torch.randint(-2, 3, (co, 3, 3, c), generator=gc).float()
    w1 = torch.randint(-2, 3, (co, 1, 1, c), generator=gc).float()
    bias = torch.randint(-8, 9, (co,), generator=gc).float()
    with Options(yv):
        for k, s_, w in ((3, 2, w3), (1, 1, w1)):
            Ho = H // s_
            assert yv.conv2d_instance(B, Ho, Ho, k, s_, c, 0, co, co, co if k == 1 else 0,
                                      yv.EPI_RES_BF16 if k == 1 else 0) == yv.CONV_DMA_64_3 | yv.CONV_STAGED
            wd = bf(w.reshape(co, k * k * c)).to(DEV)
            out_big = torch.full((B, Ho, Ho, co), SENTINEL, dtype=torch.bfloat16, device=DEV)
            out_small = torch.full_like(out_big, SENTINEL)
            fl = yv.EPI_RES_BF16 if k == 1 else 0
            yv.conv2d(yv.view(big, off, c), None, B, Ho, Ho, k, s_, wd, bias.to(DEV), out_big, 0, fl,
                      res=big if k == 1 else None, res_c_off=off if k == 1 else 0)
            yv.conv2d(yv.view(small, 0, c), None, B, Ho, Ho, k, s_, wd, bias.to(DEV), out_small, 0, fl,
                      res=small if k == 1 else None, res_c_off=0)
            torch.cuda.synchronize()
            assert torch.equal(out_big, out_small), k
            for b in (0, B - 1):
                x = small[b:b + 1].float().cpu()
                ref = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2).contiguous(), bias, stride=s_, padding=k // 2)
                ref = ref.permute(0, 2, 3, 1)
                assert float(ref.abs().max()) < 2 ** 24
                exp = bf(bf(ref).float() + x) if k == 1 else bf(ref)                   # staged epilogue: two roundings
                assert torch.equal(out_big[b:b + 1].cpu(), exp), (k, b)


# ------------------------------------------------------------------------------------------------ B.2
# (dma64_1x1_nk1, dma64_1x1_nk2_n80, dma64_stride2_1x1: one and two K steps - the four-stage ring's prologue runs out of steps)
SWEEP = ["igemm16", "igemm32_cin24", "dma64_1x1_nk1", "dma64_1x1_nk2_n80", "dma64_stride2_1x1", "dma64_3x3_cin64", "dma64_3x3_cin128", "dma64_two_src_128up_128", "dma64_33x17_cin192", "dma64_slices_3x3_s2",
         "dma64_two_src_128up_64", "dma64_two_src_slices", "dma128_b16_80x80_3x3"]


def test_every_route_agrees_on_the_same_data(yv):
    """conv_dma 0..8 x staged_epilogue {0, 1} x conv_splitk {0, 1} on the same operands: every run equals the integer reference
    of the epilogue form its route code names.  The sweep must reach all five cgemm_dma_kernel instantiations, all four igemm
    tile widths and the split-K form, with and without the staged epilogue."""
    table = {c["name"]: c for c in cases(yv)}
    seen = set()
    for name in SWEEP:
        c = table[name]
        d = to_device(c, make_data(c, seed=sum(map(ord, name)) + 1))
        exp = {(kind, st): expected(c, d, kind, st).to(DEV) for kind in KINDS for st in ((False, True) if kind == "res" else (False,))}
        for dma in range(9):
            for staged_opt in (0, 1):
                for splitk in (0, 1):
                    with Options(yv, conv_dma=dma, staged_epilogue=staged_opt, conv_splitk=splitk):
                        for kind in KINDS:
                            fl = kind_flags(yv, kind)
                            code = query(yv, c, fl)
                            seen.add(code)
                            got, outside = split_out(c, launch(yv, c, d, fl))
                            st = bool(code & yv.CONV_STAGED) and kind == "res"
                            what = (name, kind, dict(conv_dma=dma, staged_epilogue=staged_opt, conv_splitk=splitk), code)
                            assert torch.equal(got, exp[(kind, st)]), what
                            assert bool((outside == SENTINEL).all()), what
    kern = {code & 15 for code in seen}
    assert kern == set(range(9)), sorted(kern)                          # four igemm widths, five LDS-DMA instantiations
    S, K = yv.CONV_STAGED, yv.CONV_SPLITK
    for need in (yv.CONV_DMA_64_2 | S, yv.CONV_DMA_64_3 | S, yv.CONV_DMA_64_4 | S, yv.CONV_DMA_128_2 | S, yv.CONV_DMA_128_3 | S,
                 yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_64 | S, yv.CONV_IGEMM_128,
                 yv.CONV_IGEMM_128 | S, yv.CONV_IGEMM_16 | K, yv.CONV_IGEMM_32 | K, yv.CONV_IGEMM_64 | K, yv.CONV_IGEMM_128 | K,
                 yv.CONV_IGEMM_128 | S | yv.CONV_TWO, yv.CONV_IGEMM_128 | K | yv.CONV_TWO):
        assert need in seen, (need, sorted(seen))


# ------------------------------------------------------------------------------------------------ B.3
def rounding_routes(yv):
    """(what, Cout, out channel offset / stride, options, route that runs, two roundings)"""
    S, K = yv.CONV_STAGED, yv.CONV_SPLITK
    return [
        ("32-wide tiles", 32, (0, 32), {}, yv.CONV_IGEMM_32, False),
        ("staged_epilogue = 0", 64, (0, 64), dict(staged_epilogue=0), yv.CONV_IGEMM_64, False),
        ("output at channel offset 4", 64, (4, 72), {}, yv.CONV_IGEMM_64, False),
        ("split-K reduce pass", 64, (0, 64), dict(conv_splitk=1), yv.CONV_IGEMM_64 | K, False),
        ("LDS-DMA 64-wide", 64, (0, 64), {}, yv.CONV_DMA_64_3 | S, True),
        ("LDS-DMA 128-wide", 128, (0, 128), dict(conv_dma=1), yv.CONV_DMA_128_2 | S, True),
        ("igemm 64-wide staged", 64, (0, 64), dict(conv_dma=0), yv.CONV_IGEMM_64 | S, True),
        ("igemm 128-wide staged", 128, (8, 136), dict(conv_dma=0), yv.CONV_IGEMM_128 | S, True),
    ]


def test_shortcut_rounding_rule(yv):
    """bias + bf16 shortcut: the direct epilogue (and the split-K reduce pass) stores bf16(y + r); the staged epilogue rounds y to
    bf16 first and stores bf16(bf16(y) + r) (include/yv_hip.h at yv_conv2d).  Operands in [-4, 4], 3 x 3, 64 input channels,
    shortcut in [-64, 64]: |y| passes 256 often enough that the two rules differ on more than 1 % of the outputs (asserted: it is
    what makes this test able to tell them apart), and each route must equal ITS rule exactly."""
    for what, cout, out, opts, route, two in rounding_routes(yv):
        c = case(what, 2, 20, 20, 3, 1, [(64, 0, 0, 0)], cout, route, out=out, res=(8, cout + 16))
        d = to_device(c, make_data(c, seed=cout + out[0], amp=4, wamp=4, ramp=64))
        once, twice = expected(c, d, "res", False), expected(c, d, "res", True)
        differ = float((once.float() != twice.float()).float().mean())
        print(f"\n{what}: the two rounding rules differ on {100 * differ:.2f} % of {once.numel()} outputs")
        assert differ >= 0.01, (what, differ)
        with Options(yv, **opts):
            if out[0] % 8 == 0:                                             # (the query assumes aligned bases)
                assert query(yv, c, yv.EPI_RES_BF16) == route, what
            got, _ = split_out(c, launch(yv, c, d, yv.EPI_RES_BF16))
        got = got.cpu()
        assert torch.equal(got, twice if two else once), (what, "equals the OTHER rule" if torch.equal(got, once if two else twice)
                                                          else "equals neither rule")


# ------------------------------------------------------------------------------------------------ B.4
# Largest |device - float64| of SiLU on the f32 route (EPI_SILU | EPI_OUT_F32, no rounding of the output) over the
# pre-activations of silu_routes(), measured on an MI355X by test_silu_f32_route_error: see its docstring.  The gates below
# use twice that.
SILU_ABS_MEASURED = 1.14e-6
SILU_ABS = 2 * SILU_ABS_MEASURED


def silu_routes(yv):
    S, K = yv.CONV_STAGED, yv.CONV_SPLITK
    return [
        ("igemm 32-wide, direct epilogue", (2, 20, 20), 32, {}, yv.CONV_IGEMM_32),
        ("igemm 64-wide, staged epilogue", (2, 20, 20), 64, dict(conv_dma=0), yv.CONV_IGEMM_64 | S),
        ("igemm 128-wide, staged epilogue", (2, 20, 20), 144, dict(conv_dma=0), yv.CONV_IGEMM_128 | S),
        ("split-K reduce pass", (2, 20, 20), 64, dict(conv_splitk=1), yv.CONV_IGEMM_64 | K),
        ("LDS-DMA 64-wide", (2, 20, 20), 80, {}, yv.CONV_DMA_64_3 | S),
        ("LDS-DMA 128-wide", (16, 80, 80), 128, {}, yv.CONV_DMA_128_2 | S),
    ]


def silu_case(yv, what, shape, cout, route):
    """The integer operands of the parity cases with weights and bias scaled by 1/16 (exact in bf16): the pre-activation is an
    exact multiple of 1/16 in f32 and in the float64 reference alike."""
    c = case(what, *shape, 3, 1, [(64, 0, 0, 0)], cout, route, res=(8, cout + 16))
    d = make_data(c, seed=cout + shape[0], ramp=8)
    d["w"], d["bias"], d["ref"] = d["w"] / 16, d["bias"] / 16, d["ref"] / 16
    pre = d["ref"].double()
    return c, to_device(c, d), pre, pre * torch.sigmoid(pre)


def half_ulp_bf16(v):
    """Half the spacing of bf16 (8 significant bits) in the binade of |v|: 2^(floor(log2 |v|) - 8)."""
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** -120))           # |v| = m * 2^ex, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), ex - 9)


def test_silu_f32_route_error(yv):
    """EPI_SILU | EPI_OUT_F32 rounds nothing on the way out: what differs from float64 x * sigmoid(x) of the (exact)
    pre-activation is the device's silu_f (hardware exp and reciprocal) alone.  Prints the largest absolute difference per
    route.  Measured on an MI355X: 1.134e-06 over all routes (9.98e-07 .. 1.134e-06 per route, pre-activations within +-17.75,
    where one f32 step of the result is 9.5e-07 .. 1.9e-06) - recorded, rounded up, as SILU_ABS_MEASURED.  All routes call the
    same silu_f, so each must stay within twice the recorded maximum (SILU_ABS), which is also the absolute term of
    test_silu_epilogues_by_element."""
    worst = 0.0
    for what, shape, cout, opts, route in silu_routes(yv):
        c, d, pre, ref = silu_case(yv, what, shape, cout, route)
        with Options(yv, **opts):
            fl = yv.EPI_SILU | yv.EPI_OUT_F32
            assert query(yv, c, fl) == route, what
            got, _ = split_out(c, launch(yv, c, d, fl))
        err = float((got.cpu().double() - ref).abs().max())
        print(f"\n{what}: |pre| <= {float(pre.abs().max()):.2f}, silu f32 route max abs error {err:.3e}")
        worst = max(worst, err)
    print(f"\nsilu f32 route, max abs error over all routes: {worst:.3e} (recorded {SILU_ABS_MEASURED:.3e})")
    assert worst <= SILU_ABS, (worst, SILU_ABS)


@pytest.mark.parametrize("with_res", [False, True], ids=["silu", "silu_res"])
def test_silu_epilogues_by_element(yv, with_res):
    """bias -> SiLU (-> + bf16 shortcut) -> bf16 against float64, element by element, per route family.  The bound is one half-ulp
    of bf16 per rounding the route performs - one, or two where the staged epilogue adds a shortcut (test_shortcut_rounding_rule)
    - taken in the binade of the value that is rounded (2^-9 of it at the top of a binade, 2^-8 at the bottom), plus SILU_ABS for
    the device's silu_f and, with a shortcut, the rounding of its f32 addition."""
    for what, shape, cout, opts, route in silu_routes(yv):
        c, d, pre, s = silu_case(yv, what, shape, cout, route)
        fl = yv.EPI_SILU | (yv.EPI_RES_BF16 if with_res else 0)
        with Options(yv, **opts):
            assert query(yv, c, fl) == route, what
            got, outside = split_out(c, launch(yv, c, d, fl))
        assert bool((outside == SENTINEL).all()), what
        got = got.cpu().double()
        if with_res:
            r = d["res"][..., 8:8 + cout].double()
            ref = s + r
            if route & yv.CONV_STAGED:
                first = half_ulp_bf16(s.abs() + SILU_ABS)
                bound = first + half_ulp_bf16(ref.abs() + first + SILU_ABS)
            else:
                bound = half_ulp_bf16(ref.abs() + SILU_ABS)
        else:
            ref = s
            bound = half_ulp_bf16(ref.abs() + SILU_ABS)
        if with_res:
            bound = bound + ref.abs() * 2.0 ** -24                # the f32 addition of the shortcut
        err = (got - ref).abs()
        over = err - (bound + SILU_ABS)
        print(f"\n{what}: max error / bound {float((err / (bound + SILU_ABS)).max()):.3f}")
        assert bool((over <= 0).all()), (what, float(over.max()), int((over > 0).sum()))


# ------------------------------------------------------------------------------------------------ B.5
def test_instances_cover_the_bench_shapes(yv):
    """Every convolution of YOLOv8n at batch 32, YOLOv8s at batch 16 and YOLOv8m at batch 64 (640 x 640) that yv_conv2d accepts
    takes, under the shipped options, a route that test_exact_integer_parity runs - among them the 128-wide LDS-DMA instance."""
    from oracle import yolo
    from yvhip.engines import LAYER_STRIDE
    covered = covered_codes(yv)
    seen = set()
    with Options(yv):
        for scale, B in (("n", 32), ("s", 16), ("m", 64)):
            for key, cin, cout, k, s in yolo.conv_shapes(scale, 5):
                parts = key.split(".")
                idx = int(parts[1])
                st = (8, 16, 32)[int(parts[3])] if idx == 22 else LAYER_STRIDE[idx]
                H = 640 // st
                try:
                    inst = yv.conv2d_instance(B, H, H, k, s, cin, 0, cout, cout)
                except yv.YvError:                                  # the 3-channel stem, the 5-class output: not yv_conv2d's shapes
                    assert cin % 8 or cout % 4, (scale, key)
                    continue
                assert inst in covered, (scale, key, inst, sorted(covered))
                seen.add(inst)
    assert yv.CONV_DMA_128_2 | yv.CONV_STAGED in seen and yv.CONV_DMA_64_3 | yv.CONV_STAGED in seen, sorted(seen)
