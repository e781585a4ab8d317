"""The route of a bf16 convolution - kernel instance, staged epilogue, split-K - as yv_conv2d_instance reports it: the same
function the launcher calls decides it, so pinning it here (no GPU needed) pins what yv_conv2d launches.  The shipped rule
("conv_dma" = 8, "conv_splitk" = 0, "staged_epilogue" = 1) on either side of each of its thresholds, the options that change
it, and the codes of rejected arguments."""
import contextlib

import pytest

import yvhip as yv

SHIPPED = {"conv_dma": 8, "conv_splitk": 0, "staged_epilogue": 1}
ST, SK, TWO = yv.CONV_STAGED, yv.CONV_SPLITK, yv.CONV_TWO


@contextlib.contextmanager
def options(**kw):
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


def inst(B, H, W, k, s, c0, c1, cout, out_ld=None, **kw):
    return yv.conv2d_instance(B, H, W, k, s, c0, c1, cout, cout if out_ld is None else out_ld, **kw)


def test_options_are_the_shipped_ones_by_default():
    for k, v in SHIPPED.items():
        assert yv.get_option(k) == v, k


def test_codes_are_distinct():
    kerns = [yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_128, yv.CONV_DMA_64_2, yv.CONV_DMA_64_3,
             yv.CONV_DMA_64_4, yv.CONV_DMA_128_2, yv.CONV_DMA_128_3]
    assert kerns == list(range(9)) and (ST, SK, TWO) == (16, 32, 64)


def test_shipped_rule_large_maps():
    with options():
        # M = B * 80 * 80 on either side of 100,000 output pixels
        assert inst(16, 80, 80, 3, 1, 64, 0, 128) == yv.CONV_DMA_128_2 | ST            # 102,400
        assert inst(15, 80, 80, 3, 1, 64, 0, 128) == yv.CONV_DMA_64_3 | ST             # 96,000
        assert inst(1, 250, 400, 1, 1, 64, 0, 128) == yv.CONV_DMA_128_2 | ST           # exactly 100,000
        assert inst(1, 249, 400, 1, 1, 64, 0, 128) == yv.CONV_DMA_64_3 | ST
        # ... and only with more than 64 output channels
        assert inst(16, 80, 80, 3, 1, 64, 0, 64) == yv.CONV_DMA_64_3 | ST
        assert inst(16, 80, 80, 3, 1, 64, 0, 72) == yv.CONV_DMA_128_2 | ST
        # stride 2: M counts OUTPUT pixels
        assert inst(16, 80, 80, 3, 2, 64, 0, 128) == yv.CONV_DMA_128_2 | ST
        assert inst(16, 40, 40, 3, 2, 64, 0, 128) == yv.CONV_DMA_64_3 | ST


def test_shipped_rule_eligibility_of_the_lds_dma_route():
    with options():
        assert inst(2, 20, 20, 3, 1, 64, 0, 64) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 20, 20, 3, 1, 32, 0, 64) == yv.CONV_IGEMM_64 | ST               # Cin 32: a K step straddles taps
        assert inst(2, 20, 20, 3, 1, 192, 0, 64) == yv.CONV_DMA_64_3 | ST              # not a power of two, a multiple of 64
        assert inst(2, 20, 20, 3, 1, 96, 0, 64) == yv.CONV_IGEMM_64 | ST
        assert inst(2, 20, 20, 3, 1, 64, 0, 60) == yv.CONV_IGEMM_64                    # Cout < 64 (and not a multiple of 8)
        assert inst(2, 20, 20, 3, 1, 64, 0, 56) == yv.CONV_IGEMM_64 | ST
        # two sources: both on 64-channel boundaries, or igemm's two-source instantiation
        assert inst(2, 20, 20, 1, 1, 64, 64, 64) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 20, 20, 1, 1, 128, 64, 128) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 20, 20, 1, 1, 32, 96, 64) == yv.CONV_IGEMM_64 | ST | TWO        # Cin 128, but c0 % 64 != 0
        assert inst(2, 20, 20, 1, 1, 32, 16, 24) == yv.CONV_IGEMM_32 | TWO


def test_igemm_tile_widths():
    with options():
        for cout, code in ((8, yv.CONV_IGEMM_16), (16, yv.CONV_IGEMM_16), (24, yv.CONV_IGEMM_32), (32, yv.CONV_IGEMM_32),
                           (40, yv.CONV_IGEMM_64 | ST), (64, yv.CONV_IGEMM_64 | ST), (72, yv.CONV_IGEMM_128 | ST),
                           (256, yv.CONV_IGEMM_128 | ST)):
            assert inst(2, 12, 12, 3, 1, 24, 0, cout) == code, cout


def test_alignment_decides_the_staged_epilogue():
    with options():
        # bf16 rows need a stride that is a multiple of 8 elements; without the staged epilogue there is no LDS-DMA route
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, out_ld=72) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, out_ld=68) == yv.CONV_IGEMM_64
        assert inst(2, 20, 20, 3, 1, 64, 0, 128, out_ld=132) == yv.CONV_IGEMM_128
        assert inst(2, 20, 20, 3, 1, 64, 0, 68) == yv.CONV_IGEMM_128                    # Cout not a multiple of 8
        # f32 rows: a multiple of 4
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, out_ld=68, flags=yv.EPI_OUT_F32) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 20, 20, 3, 1, 64, 0, 68, flags=yv.EPI_OUT_F32) == yv.CONV_DMA_64_3 | ST
        # the residual's stride counts too
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, res_ld=64, flags=yv.EPI_RES_BF16) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, res_ld=68, flags=yv.EPI_RES_BF16) == yv.CONV_IGEMM_64
    with options(staged_epilogue=0):
        assert inst(2, 20, 20, 3, 1, 64, 0, 64) == yv.CONV_IGEMM_64
        assert inst(16, 80, 80, 3, 1, 64, 0, 128) == yv.CONV_IGEMM_128


# (M, Cout, K) corners: small map / deep K, small map / shallow K, large map
DMA_SHAPES = {"deep": (2, 20, 20, 3, 1, 128), "shallow": (2, 20, 20, 3, 1, 64), "large": (16, 80, 80, 3, 1, 64)}
DMA_TABLE = {   # conv_dma -> {(shape, Cout): kernel instance}
    1: {("deep", 128): 7, ("deep", 64): 4, ("shallow", 128): 7, ("large", 128): 7, ("large", 64): 4},
    2: {("deep", 128): 5, ("deep", 64): 5, ("shallow", 128): 5, ("large", 128): 5, ("large", 64): 5},
    3: {("deep", 128): 8, ("deep", 64): 5, ("shallow", 128): 8, ("large", 128): 8, ("large", 64): 5},
    4: {("deep", 128): 6, ("deep", 64): 6, ("shallow", 128): 6, ("large", 128): 6, ("large", 64): 6},
    5: {("deep", 128): 5, ("deep", 64): 5, ("shallow", 128): 7, ("shallow", 64): 4, ("large", 128): 7, ("large", 64): 4},
    6: {("deep", 128): 5, ("deep", 64): 5, ("shallow", 128): 4, ("shallow", 64): 4, ("large", 128): 4},
    7: {("deep", 128): 5, ("shallow", 128): 5, ("large", 128): 7, ("large", 64): 4},
    8: {("deep", 128): 5, ("shallow", 128): 5, ("large", 128): 7, ("large", 64): 5},
}


@pytest.mark.parametrize("mode", sorted(DMA_TABLE))
def test_every_conv_dma_value(mode):
    with options(conv_dma=mode):
        for (shape, cout), kern in DMA_TABLE[mode].items():
            assert inst(*DMA_SHAPES[shape], 0, cout) == kern | ST, (mode, shape, cout)


def test_conv_dma_off_sends_everything_to_igemm():
    with options(conv_dma=0):
        assert inst(16, 80, 80, 3, 1, 64, 0, 128) == yv.CONV_IGEMM_128 | ST
        assert inst(2, 20, 20, 3, 1, 64, 0, 64) == yv.CONV_IGEMM_64 | ST
        assert inst(2, 20, 20, 1, 1, 128, 64, 128) == yv.CONV_IGEMM_128 | ST | TWO
        assert inst(2, 20, 20, 1, 1, 640, 0, 144) == yv.CONV_IGEMM_128 | ST


def test_splitk_needs_the_option_and_a_workspace():
    shape = (2, 20, 20, 3, 1, 128, 0, 128)            # 7 tiles, 18 K steps: 8 slices of 800 x 128 f32 partials = 3,276,800 bytes
    with options():
        assert inst(*shape) == yv.CONV_DMA_64_3 | ST
    with options(conv_splitk=1):
        assert inst(*shape) == yv.CONV_IGEMM_128 | SK                                   # no staged epilogue, no LDS-DMA route
        assert inst(*shape, ws_bytes=8 * 800 * 128 * 4) == yv.CONV_IGEMM_128 | SK
        assert inst(*shape, ws_bytes=8 * 800 * 128 * 4 - 1) == yv.CONV_DMA_64_3 | ST     # the split is not shrunk to fit
        assert inst(*shape, ws_bytes=0) == yv.CONV_DMA_64_3 | ST
        assert inst(2, 10, 12, 3, 1, 32, 0, 16) == yv.CONV_IGEMM_16 | SK                # 5 K steps: two slices
        assert inst(2, 20, 20, 1, 1, 64, 0, 64) == yv.CONV_DMA_64_3 | ST                # one K step: nothing to split
        assert inst(2, 20, 20, 1, 1, 32, 96, 64) == yv.CONV_IGEMM_64 | ST | TWO         # two K steps: at most one slice
        assert inst(2, 20, 20, 1, 1, 32, 224, 64) == yv.CONV_IGEMM_64 | SK | TWO        # four K steps: two slices
        assert inst(16, 80, 80, 3, 1, 64, 0, 128) == yv.CONV_DMA_128_2 | ST             # 800 tiles: no split


def test_rejected_arguments_return_the_codes_of_yv_conv2d():
    q = yv.lib.yv_conv2d_instance
    ok = dict(B=2, H=20, W=20, k=3, s=1, c0=64, c1=0, cout=64, out_ld=64, res_ld=0, flags=yv.EPI_BIAS, ws=0)

    def code(**kw):
        a = dict(ok, **kw)
        return q(a["B"], a["H"], a["W"], a["k"], a["s"], a["c0"], a["c1"], a["cout"], a["out_ld"], a["res_ld"], a["flags"], a["ws"])

    with options():
        assert code() == yv.CONV_DMA_64_3 | ST
        for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(cout=0), dict(k=5), dict(k=2), dict(s=3), dict(s=0), dict(c0=12),
                    dict(c0=0), dict(c1=-8), dict(k=1, c1=12), dict(c1=64), dict(cout=6), dict(out_ld=66),
                    dict(flags=yv.EPI_BIAS | yv.EPI_RES_BF16, res_ld=6), dict(flags=yv.EPI_BIAS | yv.EPI_GELU),
                    dict(flags=yv.EPI_BIAS | yv.EPI_RES_F32), dict(flags=yv.EPI_BIAS | yv.EPI_POSEMB)):
            assert code(**bad) == -1, bad                                                # YV_ERR_ARG
        assert code(k=1, c1=64) == yv.CONV_DMA_64_3 | ST                                 # two sources are a property of 1 x 1
        assert code(B=1, H=40000, W=40000, c0=8, cout=8, out_ld=8) == -2                 # YV_ERR_LIMIT: one image beyond 2 GB
        assert code(B=3, H=30000, W=30000, k=1, c0=8, cout=8, out_ld=8) == -2            # more than 2^31 - 1 output pixels
        assert code(c0=4096, cout=32768, out_ld=32768) == -2                             # weights beyond 2 GB
    with pytest.raises(yv.YvError):
        yv.conv2d_instance(2, 20, 20, 5, 1, 64, 0, 64, 64)


def test_query_leaves_the_options_alone():
    before = {k: yv.get_option(k) for k in SHIPPED}
    with options(conv_dma=3, conv_splitk=1, staged_epilogue=0):
        inst(2, 20, 20, 3, 1, 128, 0, 128)
    assert {k: yv.get_option(k) for k in SHIPPED} == before
