"""The LDS-DMA convolution for 32-aligned input channels (cgemm_dma32_kernel<64, 4, 1, 3> and <128, 2, 2, 2>, the two shipped
instances; option "conv_dma32") against the exact integer reference of tests/test_gpu_conv_routes.py: integer operands with
loud borders in every channel of the buffer, outputs prefilled with 0.5, torch.equal against F.conv2d in fp32.  Every case runs
on each instance, forced in turn with "conv_dma32_cols", asserts its route code before it runs, and is compared bit for bit with the
parent route ("conv_dma32" = 0, an igemm_kernel code) on the same data.

Both instances and the parent's 64- and 128-wide igemm_kernel tiles run the staged epilogue (a bf16 shortcut is added to the
rounded activation: two roundings, include/yv_hip.h at yv_conv2d).  The parity cases nevertheless use operands in [-1, 1] and
assert |y| < 256, where bf16 holds every integer and one and two roundings give the same exact integer, so the comparison with
the parent route does not rest on which epilogue either side takes."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_routes import DEV, SENTINEL, Options, bf, case, check_exact, kind_flags, launch, make_data, query, split_out, to_device

pytestmark = pytest.mark.gpu
COLS = (64, 128)


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def new_code(yv, cols):
    return {64: yv.CONV_DMA32_64 | yv.CONV_STAGED, 128: yv.CONV_DMA32_128 | yv.CONV_STAGED}[cols]


def is_igemm(yv, code):
    return code & 15 in (yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_128) and not code & yv.CONV_SPLITK


def cases():
    S = 0          # `expect` is filled per instance
    return [
        # 27 blocks of 32 channels: 13 full K steps and a half step, the tap changing inside a step
        case("m35_3x3_cin96_n64", 1, 5, 7, 3, 1, [(96, 0, 0, 0)], 64, S),
        # a tile spans two images; the second column tile is partial at 64 wide, the only one at 128 wide
        case("m70_3x3_cin96_n96", 2, 5, 7, 3, 1, [(96, 0, 0, 0)], 96, S),
        case("m35_1x1_cin32_one_block", 1, 5, 7, 1, 1, [(32, 0, 0, 0)], 64, S),      # the only step is a half step
        case("m70_1x1_cin96_n72", 2, 5, 7, 1, 1, [(96, 0, 0, 0)], 72, S),            # three blocks, a ragged N
        case("m81_1x1_cin160_n128", 1, 9, 9, 1, 1, [(160, 0, 0, 0)], 128, S),        # five blocks
        case("m81_3x3_cin288_n288", 1, 9, 9, 3, 1, [(288, 0, 0, 0)], 288, S),        # 81 blocks: the ring wraps many times
        case("m162_3x3_stride2_cin96_n192", 2, 9, 9, 3, 2, [(96, 0, 0, 0)], 192, S), # model.3's class, an odd extent
        case("m35_3x3_stride2_cin32", 1, 5, 7, 3, 2, [(32, 0, 0, 0)], 64, S),
        # two sources: the boundary inside a K step; inside step 0 (an upsampled source: even extents)
        case("m80_two_src_96up_32", 1, 8, 10, 1, 1, [(96, 1, 0, 0), (32, 0, 0, 0)], 64, S),
        case("m80_two_src_32_96up_n128", 1, 8, 10, 1, 1, [(32, 0, 0, 0), (96, 1, 0, 0)], 128, S),
        # the engine's C2f slices: a bottleneck of model.4 in its 576-wide concat buffer, of model.8 in its 1,152-wide one
        case("m81_c2f_slices_cin96", 1, 9, 9, 3, 1, [(96, 0, 96, 576)], 96, S, out=(192, 576), res=(96, 576)),
        case("m35_c2f_slices_cin288", 1, 5, 7, 3, 1, [(288, 0, 288, 1152)], 288, S, out=(576, 1152), res=(288, 1152)),
    ]


CASES = {c["name"]: c for c in cases()}
_DATA = {}


def parity_data(name):
    """The case's integer data in [-1, 1] (made once, shared by the instances) with |y| < 256 asserted on the CPU."""
    if name not in _DATA:
        d = make_data(CASES[name], seed=sum(map(ord, name)), amp=1, wamp=1, ramp=64)
        assert float(d["ref"].abs().max()) < 256, name
        _DATA[name] = to_device(CASES[name], d)
    return _DATA[name]


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_integer_parity(yv, name, cols):
    """bias -> bf16, bias -> f32 and bias + bf16 shortcut, element for element, on the instance the options force; the parent route
    (igemm_kernel) on the same data gives the same bits."""
    code = new_code(yv, cols)
    c = dict(CASES[name], expect=code, query=code)
    d = parity_data(name)
    for kind in ("bf16", "f32", "res"):
        fl = kind_flags(yv, kind)
        with Options(yv, conv_dma32=1, conv_dma32_cols=cols):
            assert query(yv, c, fl) == code, (name, kind)
            check_exact(yv, c, d, kind, staged=bool(code & yv.CONV_STAGED), what=f"cols {cols}")
            got = launch(yv, c, d, fl)
        with Options(yv, conv_dma32=0):
            assert is_igemm(yv, query(yv, c, fl)), (name, kind)
            parent = launch(yv, c, d, fl)
        assert torch.equal(got, parent), (name, kind, cols)


@pytest.mark.parametrize("cols", COLS)
def test_silu_equals_the_parent_route_bit_for_bit(yv, cols):
    """bias -> SiLU -> bf16 and -> f32 on integer operands scaled by 1/16 (exact pre-activations): both routes call the same
    silu_f on the same f32 value, so the bits are equal - and the channels outside the output slice keep the sentinel."""
    for name in ("m81_c2f_slices_cin96", "m70_1x1_cin96_n72", "m80_two_src_96up_32", "m35_1x1_cin32_one_block"):
        c = dict(CASES[name], expect=new_code(yv, cols))
        d = make_data(c, seed=len(name))
        d["w"], d["bias"] = d["w"] / 16, d["bias"] / 16
        d = to_device(c, d)
        for fl in (yv.EPI_SILU, yv.EPI_SILU | yv.EPI_OUT_F32):
            with Options(yv, conv_dma32=1, conv_dma32_cols=cols):
                assert query(yv, c, fl) == c["expect"], name
                got = launch(yv, c, d, fl)
            with Options(yv, conv_dma32=0):
                assert is_igemm(yv, query(yv, c, fl)), name
                parent = launch(yv, c, d, fl)
            assert torch.equal(got, parent), (name, cols, fl)
            inside, outside = split_out(c, got)
            assert bool((outside == SENTINEL).all()), (name, cols, fl)
            assert not bool((inside == SENTINEL).all())


def random_case(yv, cin, cout, cols, seed):
    B, H, W = 1, 9, 9
    K = 9 * cin
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(B, H, W, cin, generator=g))
    w = bf(torch.randn(cout, 3, 3, cin, generator=g) * 0.05)
    bias = torch.randn(cout, generator=g)
    c = case("random", B, H, W, 3, 1, [(cin, 0, 0, 0)], cout, new_code(yv, cols))
    d = dict(bufs_d=[x.to(DEV)], w_d=w.reshape(cout, K).to(DEV), bias_d=bias.to(DEV), res_d=None)
    return c, d, x, w, bias


@pytest.mark.parametrize("cols", COLS)
def test_the_launch_does_not_change_the_result(yv, cols):
    """Two launches on random data give the same bits."""
    c, d, *_ = random_case(yv, 96, 96, cols, 3)
    with Options(yv, conv_dma32=1, conv_dma32_cols=cols):
        assert query(yv, c, 0) == new_code(yv, cols)
        a, b = launch(yv, c, d, 0), launch(yv, c, d, 0)
    assert torch.equal(a, b)


_FP64 = {}


def fp64_reference(cin):
    """(case data, fp64 reference, bound) of the random 3 x 3 layer of `cin` channels, computed once for the instances."""
    if cin not in _FP64:
        import yvhip
        c, d, x, w, bias = random_case(yvhip, cin, cin, 64, 11 + cin)
        K = 9 * cin
        xin, wk = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
        ref = (F.conv2d(xin, wk, bias.double(), padding=1)).permute(0, 2, 3, 1)
        S = (F.conv2d(xin.abs(), wk.abs(), bias.double().abs(), padding=1)).permute(0, 2, 3, 1)
        _FP64[cin] = (c, d, ref, 2.0 ** -8 * ref.abs() + 2 * K * 2.0 ** -24 * S)
    return _FP64[cin]


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("cin", (96, 288))
def test_random_data_against_fp64(yv, cin, cols):
    """3 x 3, Cin = Cout = 96 and 288, 9 x 9, bias only, bf16 out, against the fp64 convolution of the bf16 operands.  Every
    element is gated at 2^-8 |ref| + 2 K 2^-24 S, S the fp64 convolution of the absolute values: one bf16 rounding of the result
    (half a spacing is at most 2^-8 of the value) plus f32 accumulation of K products in any order (each partial sum is below S
    and is rounded to 2^-24 of itself at most once per addition, the bias addition included in the factor 2) - the bound
    tests/test_gpu_conv_small.py derives.  Whether the bits equal the parent route's on random data is printed, not asserted."""
    c, d, ref, bound = fp64_reference(cin)
    with Options(yv, conv_dma32=1, conv_dma32_cols=cols):
        assert query(yv, c, 0) == new_code(yv, cols)
        got = launch(yv, c, d, 0)
    with Options(yv, conv_dma32=0):
        assert is_igemm(yv, query(yv, c, 0))
        parent = launch(yv, c, d, 0)
    err = (got.cpu().double() - ref).abs()
    differ = int((got != parent).sum())
    print(f"\ncin {cin} cols {cols}: max error / bound {float((err / bound).max()):.3f}; "
          f"{differ} of {got.numel()} values differ from the parent route's")
    assert bool((err <= bound).all()), (cin, cols, float((err / bound).max()))


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


@pytest.mark.parametrize("cols", COLS)
def test_engine_with_the_flag_against_the_oracle(yv, cols, monkeypatch):
    """YoloEngine("m", nc=80, size=64, dma32=True) at one image with the instance forced: the gates of
    test_gpu_models.py::test_yolo_engine_vs_oracle for ("m", 80, 64, 1), and as many launches on a new code as
    engines.dma32_layers names.  The distance to the unflagged engine is printed, not gated."""
    from oracle import yolo as oy
    from yvhip import engines
    scale, nc, size, B = "m", 80, 64, 1
    sd = oy.init_state(scale, nc, seed=7)
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (B, size, size, 3), generator=g, dtype=torch.uint8)
    raw, outs = oy.forward_raw(sd, oy.blob(img), scale, nc, return_feats=True)
    plain = engines.YoloEngine(sd, scale, nc, size)
    pb, pc = [[t.clone() for t in part] for part in plain.forward_raw(img.to(DEV))]
    eng = engines.YoloEngine(sd, scale, nc, size, dma32=True)
    assert eng.dma32 and not plain.dma32 and eng.resized(size).dma32
    taken = []
    conv2d = engines.conv2d

    def counting(in0, in1, B_, Ho, Wo, k, s, weight, bias, out, out_c_off, flags, res=None, res_c_off=0):
        code = yv.conv2d_instance(B_, Ho, Wo, k, s, in0.c, in1.c if in1 is not None else 0, weight.shape[0], out.shape[-1],
                                  0 if res is None else res.shape[-1], flags)
        taken.append(code)
        return conv2d(in0, in1, B_, Ho, Wo, k, s, weight, bias, out, out_c_off, flags, res=res, res_c_off=res_c_off)

    monkeypatch.setattr(engines, "conv2d", counting)
    new = (yv.CONV_DMA32_64, yv.CONV_DMA32_96, yv.CONV_DMA32_128)
    with Options(yv, conv_dma32_cols=cols):
        assert yv.get_option("conv_dma32") == 0
        box_l, cls_l = eng.forward_raw(img.to(DEV))
        torch.cuda.synchronize()
        assert yv.get_option("conv_dma32") == 0                     # restored
        with Options(yv, conv_dma32=1, conv_dma32_cols=cols):
            want = engines.dma32_layers(scale, nc, B, (size, size))
    assert want and [c & 15 for c in taken if c & 15 in new] == [new_code(yv, cols) & 15] * len(want)
    bufs = eng._buffers(B)
    for idx in (0, 1, 2, 4, 6, 9, 12, 15, 18, 21):
        got = bufs["out"][idx].float().permute(0, 3, 1, 2).cpu()
        assert rel_l2(got, outs[idx]) < 2e-2, idx
    a0 = 0
    for s, st in enumerate((8, 16, 32)):
        w = size // st
        part = raw[:, :, a0:a0 + w * w].reshape(B, 64 + nc, w, w)
        assert rel_l2(box_l[s].permute(0, 3, 1, 2).cpu(), part[:, :64]) < 2e-2
        assert rel_l2(cls_l[s][..., :nc].permute(0, 3, 1, 2).cpu(), part[:, 64:]) < 2e-2
        a0 += w * w
        for what, a, b in (("box", box_l[s], pb[s]), ("cls", cls_l[s], pc[s])):
            print(f"\ncols {cols} level {s} {what}: rel-L2 to the unflagged engine {rel_l2(a, b):.2e}, "
                  f"{int((a != b).sum())} of {a.numel()} values differ")
    monkeypatch.setattr(engines, "conv2d", conv2d)
    with Options(yv, conv_dma32_cols=cols):
        eb, es = oy.decode(raw, nc, size)
        gb, gs = eng(img.to(DEV))
    assert rel_l2(gs.cpu(), es) < 2e-2
    assert float((gb.cpu() - eb).abs().max()) < 0.02 * size
