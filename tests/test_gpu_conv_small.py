"""The small-map convolution (cgemm_small_kernel<64, 2> and <32, 4>, option "conv_small") against the exact integer reference
of tests/test_gpu_conv_routes.py: integer operands with loud borders in every channel of the buffer, outputs prefilled with
0.5, torch.equal against F.conv2d in fp32.  Every case runs on both instances, forced in turn with "conv_small_rows", asserts
its route code before it runs, and is compared bit for bit with the parent route ("conv_small" = 0) on the same data.

The kernel takes the direct epilogue: with a bf16 shortcut it stores bf16(y + r), one rounding (include/yv_hip.h at yv_conv2d),
where the 128-row LDS-DMA route rounds y first.  The parity cases use operands in [-1, 1] and assert |y| < 256, where bf16 holds
every integer: both rules then give the same exact integer and the two routes can be compared bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_routes import DEV, SENTINEL, Options, bf, case, check_exact, kind_flags, launch, make_data, query, split_out, to_device

pytestmark = pytest.mark.gpu
ROWS = (64, 32)
ON = dict(conv_small=1 << 20, conv_small_fill=1 << 20)       # every eligible shape takes the step; "conv_small_rows" picks the instance


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def small_code(yv, rows):
    return yv.CONV_SMALL_64 if rows == 64 else yv.CONV_SMALL_32


def cases():
    S = 0          # `expect` is filled per instance
    return [
        # 5 x 7 = 35 pixels: one partial 64-pixel tile / one full and one partial 32-pixel tile; B = 2: a tile spans two images
        case("m35_3x3_cin64", 1, 5, 7, 3, 1, [(64, 0, 0, 0)], 64, S),                 # 9 K steps: odd for the halves, 2 x 4 + 1
        case("m70_3x3_cin64_n72", 2, 5, 7, 3, 1, [(64, 0, 0, 0)], 72, S),             # partial column tile
        case("m35_1x1_nk1", 1, 5, 7, 1, 1, [(64, 0, 0, 0)], 64, S),                   # one K step: the other groups add zeros
        case("m70_1x1_nk2_n128", 2, 5, 7, 1, 1, [(128, 0, 0, 0)], 128, S),            # two steps
        # 9 x 9 = 81 pixels: a partial second / third tile
        case("m81_3x3_cin128_n128", 1, 9, 9, 3, 1, [(128, 0, 0, 0)], 128, S),         # 18 steps
        case("m81_1x1_nk3_n72", 1, 9, 9, 1, 1, [(192, 0, 0, 0)], 72, S),              # 3 steps: one group of four idles
        case("m162_3x3_stride2", 2, 9, 9, 3, 2, [(64, 0, 0, 0)], 64, S),
        case("m35_3x3_stride2_n72", 1, 5, 7, 3, 2, [(128, 0, 0, 0)], 72, S),
        case("m80_two_src_64up_64", 1, 8, 10, 1, 1, [(64, 1, 0, 0), (64, 0, 0, 0)], 64, S),   # (an upsampled source: even extents)
        case("m160_two_src_64_128up_n128", 2, 8, 10, 1, 1, [(64, 0, 0, 0), (128, 1, 0, 0)], 128, S),
        # a source read at a channel offset with a wider pixel stride; an output at a channel offset into a wider buffer
        case("m81_slices_3x3", 1, 9, 9, 3, 1, [(64, 0, 8, 136)], 64, S, out=(8, 88), res=(16, 96)),
        case("m70_slices_1x1_n72", 2, 5, 7, 1, 1, [(64, 0, 72, 144)], 72, S, out=(24, 104), res=(80, 160)),
        case("m80_two_src_slices", 1, 8, 10, 1, 1, [(64, 1, 8, 80), (64, 0, 64, 136)], 72, S, out=(8, 96), res=(8, 88)),
    ]


CASES = {c["name"]: c for c in cases()}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_integer_parity(yv, name, rows):
    """bias -> bf16, bias -> f32 and bias + bf16 shortcut, element for element, on the instance the options force; the parent route
    on the same data gives the same bits (operands in [-1, 1]: |y| < 256, so one and two roundings of the shortcut agree)."""
    c = dict(CASES[name], expect=small_code(yv, rows), query=small_code(yv, rows))
    d = to_device(c, make_data(c, seed=sum(map(ord, name)), amp=1, wamp=1, ramp=64))
    assert float(d["ref"].abs().max()) < 256
    for kind in ("bf16", "f32", "res"):
        fl = kind_flags(yv, kind)
        with Options(yv, conv_small_rows=rows, **ON):
            assert query(yv, c, fl) == c["expect"], (name, kind)
            check_exact(yv, c, d, kind, staged=False, what=f"rows {rows}")
            got = launch(yv, c, d, fl)
        with Options(yv, conv_small=0):
            assert query(yv, c, fl) == (yv.CONV_DMA_64_3 | yv.CONV_STAGED), (name, kind)
            parent = launch(yv, c, d, fl)
        assert torch.equal(got, parent), (name, kind, rows)


@pytest.mark.parametrize("rows", ROWS)
def test_silu_equals_the_128_row_route_bit_for_bit(yv, rows):
    """bias -> SiLU -> bf16 and -> f32 on integer operands scaled by 1/16 (exact pre-activations): both routes call the same
    silu_f on the same f32 value, so the bits are equal - and the channels outside the output slice keep the sentinel."""
    for name in ("m81_3x3_cin128_n128", "m70_3x3_cin64_n72", "m80_two_src_slices", "m35_1x1_nk1"):
        c = dict(CASES[name], expect=small_code(yv, rows))
        d = make_data(c, seed=len(name))
        d["w"], d["bias"] = d["w"] / 16, d["bias"] / 16
        d = to_device(c, d)
        for fl in (yv.EPI_SILU, yv.EPI_SILU | yv.EPI_OUT_F32):
            with Options(yv, conv_small_rows=rows, **ON):
                assert query(yv, c, fl) == c["expect"], name
                got = launch(yv, c, d, fl)
            with Options(yv, conv_small=0):
                assert query(yv, c, fl) == (yv.CONV_DMA_64_3 | yv.CONV_STAGED), name
                parent = launch(yv, c, d, fl)
            assert torch.equal(got, parent), (name, rows, fl)
            _, outside = split_out(c, got)
            assert bool((outside == SENTINEL).all()), (name, rows, fl)
            assert not bool((split_out(c, got)[0] == SENTINEL).all())


@pytest.mark.parametrize("rows", ROWS)
def test_the_launch_does_not_change_the_result(yv, rows):
    """The partial tiles are added in one fixed order: two launches on random data give the same bits."""
    c = dict(CASES["m81_3x3_cin128_n128"])
    g = torch.Generator().manual_seed(3)
    x = bf(torch.randn(1, 9, 9, 128, generator=g)).to(DEV)
    w = bf(torch.randn(128, 9 * 128, generator=g) * 0.03).to(DEV)
    d = dict(bufs_d=[x], w_d=w, bias_d=torch.randn(128, generator=g).to(DEV), res_d=None)
    with Options(yv, conv_small_rows=rows, **ON):
        assert query(yv, c, 0) == small_code(yv, rows)
        a, b = launch(yv, c, d, 0), launch(yv, c, d, 0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("rows", ROWS)
def test_random_data_against_fp64(yv, rows):
    """3 x 3, Cin 128, Cout 64, 9 x 9, bias only, bf16 out, against the fp64 convolution of the bf16 operands.  Every element is
    gated at 2^-8 |ref| + 2 K 2^-24 S, S the fp64 convolution of the absolute values: one bf16 rounding of the result (half a
    spacing is at most 2^-8 of the value) plus f32 accumulation of K products in any order (each partial sum is below S and is
    rounded to 2^-24 of itself at most once per addition, the bias addition and the exchange included in the factor 2)."""
    B, H, W, cin, cout = 1, 9, 9, 128, 64
    K = 9 * cin
    g = torch.Generator().manual_seed(11 + rows)
    x = bf(torch.randn(B, H, W, cin, generator=g))
    w = bf(torch.randn(cout, 3, 3, cin, generator=g) * 0.05)
    bias = torch.randn(cout, generator=g)
    xin, wk = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    ref = (F.conv2d(xin, wk, bias.double(), padding=1)).permute(0, 2, 3, 1)
    S = (F.conv2d(xin.abs(), wk.abs(), bias.double().abs(), padding=1)).permute(0, 2, 3, 1)
    bound = 2.0 ** -8 * ref.abs() + 2 * K * 2.0 ** -24 * S
    c = case("random", B, H, W, 3, 1, [(cin, 0, 0, 0)], cout, small_code(yv, rows))
    d = dict(bufs_d=[x.to(DEV)], w_d=w.reshape(cout, K).to(DEV), bias_d=bias.to(DEV), res_d=None)
    with Options(yv, conv_small_rows=rows, **ON):
        assert query(yv, c, 0) == small_code(yv, rows)
        got = launch(yv, c, d, 0)
    err = (got.cpu().double() - ref).abs()
    print(f"\nrows {rows}: max error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (rows, float((err / bound).max()))
