"""The small-map step of conv_route ("conv_small", "conv_small_fill"; cgemm_small_kernel<64, 2> = CONV_SMALL_64 and <32, 4> =
CONV_SMALL_32) as yv_conv2d_instance reports it, without a GPU: off by default and then the route tests/test_conv_routes_cpu.py
pins; with the option on, the shapes it is for, either side of each bound, every ineligible shape on its old code, its place
ahead of split-K, and the training routes untouched.  Without a device the fill rule counts 256 CUs."""
import contextlib

import pytest

import yvhip as yv
from yvhip import engines

SHIPPED = {"conv_dma": 8, "conv_splitk": 0, "staged_epilogue": 1, "conv_small": 0, "conv_small_rows": 0}
ST, SK, TWO = yv.CONV_STAGED, yv.CONV_SPLITK, yv.CONV_TWO
S64, S32, D64 = yv.CONV_SMALL_64, yv.CONV_SMALL_32, yv.CONV_DMA_64_3 | yv.CONV_STAGED
SMALL = (S64, S32)
CUS = 256                    # what the route assumes where no device is present


@contextlib.contextmanager
def options(**kw):
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


def n_cus():
    """The CU count the fill rule uses: the device's, 256 on a host without one."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else CUS


QUERIES = [((2, 20, 20, 3, 1, 64, 0, 64), D64), ((2, 20, 20, 3, 1, 32, 0, 64), yv.CONV_IGEMM_64 | ST),
           ((2, 20, 20, 1, 1, 128, 64, 128), D64), ((2, 20, 20, 1, 1, 32, 96, 64), yv.CONV_IGEMM_64 | ST | TWO),
           ((16, 80, 80, 3, 1, 64, 0, 128), yv.CONV_DMA_128_2 | ST), ((1, 20, 20, 3, 1, 128, 0, 128), D64),
           ((2, 12, 12, 3, 1, 24, 0, 16), yv.CONV_IGEMM_16)]


def test_codes():
    assert (S64, S32) == (9, 10)
    old = [yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_128, yv.CONV_DMA_64_2, yv.CONV_DMA_64_3,
           yv.CONV_DMA_64_4, yv.CONV_DMA_128_2, yv.CONV_DMA_128_3]
    assert len(set(old + [S64, S32])) == 11 and max(S64, S32) < ST


def test_off_by_default_and_then_the_pinned_routes():
    assert yv.get_option("conv_small") == 0 and yv.get_option("conv_small_rows") == 0
    assert yv.get_option("conv_small_fill") > 0
    for shape, code in QUERIES:
        assert inst(*shape) == code, shape
    with options(conv_small=0, conv_small_fill=1 << 20, conv_small_rows=64):          # the other two keys alone switch nothing on
        for shape, code in QUERIES:
            assert inst(*shape) == code, shape


def test_shipped_shapes_take_the_new_codes():
    """The engine's bound and the shipped fill: model.8's bottleneck at one image, model.12's two-source cv1, a stride-2 layer."""
    assert engines.SMALL_MAP_PIXELS > 0
    with options(conv_small=engines.SMALL_MAP_PIXELS):
        assert inst(1, 20, 20, 3, 1, 128, 0, 128) in SMALL
        assert inst(1, 40, 40, 1, 1, 256, 128, 128) in SMALL
        assert inst(1, 20, 20, 3, 2, 128, 0, 256) in SMALL
        # the direct epilogue runs: no staged bit, no split, no two-source bit
        for shape in ((1, 20, 20, 3, 1, 128, 0, 128), (1, 40, 40, 1, 1, 256, 128, 128)):
            assert inst(*shape) & ~15 == 0
        assert inst(32, 80, 80, 3, 1, 64, 0, 128) == yv.CONV_DMA_128_2 | ST           # batch 32: far outside


def test_either_side_of_the_m_bound():
    with options(conv_small=400, conv_small_fill=1 << 20):
        assert inst(1, 20, 20, 3, 1, 128, 0, 128) in SMALL                             # M = 400
        assert inst(1, 20, 21, 3, 1, 128, 0, 128) == D64                               # M = 420
    with options(conv_small=399, conv_small_fill=1 << 20):
        assert inst(1, 20, 20, 3, 1, 128, 0, 128) == D64


def test_either_side_of_the_fill_bound():
    """tiles of 128 x 64 against fill / 8 of the CU count: 8 x 16 t pixels and one column tile make t tiles."""
    t1 = n_cus() // 8                                                                  # "conv_small_fill" = 1: at most CUs / 8 tiles
    with options(conv_small=1 << 20, conv_small_fill=1):
        assert inst(1, 8, 16 * t1, 3, 1, 64, 0, 64) in SMALL                           # on the bound
        assert inst(1, 8, 16 * (t1 + 1), 3, 1, 64, 0, 64) == D64
        assert inst(1, 8, 16 * (t1 // 2), 3, 1, 64, 0, 128) in SMALL                   # two column tiles count twice
        assert inst(1, 8, 16 * (t1 // 2 + 1), 3, 1, 64, 0, 128) == D64
    with options(conv_small=1 << 20, conv_small_fill=2):
        assert inst(1, 8, 16 * (t1 + 1), 3, 1, 64, 0, 64) in SMALL
        assert inst(1, 8, 16 * (2 * t1 + 1), 3, 1, 64, 0, 64) == D64
    if n_cus() == 256:
        # 1 x 40 x 40 -> Cout 128: 13 row tiles x 2 column tiles = 26 of the 32 that fill = 1 allows; Cout 192: 39
        with options(conv_small=1 << 20, conv_small_fill=1):
            assert inst(1, 40, 40, 3, 1, 64, 0, 128) in SMALL and inst(1, 40, 40, 3, 1, 64, 0, 192) == D64
        # the shipped fill of 5: 160 tiles
        with options(conv_small=1 << 20):
            assert inst(1, 8, 16 * 160, 3, 1, 64, 0, 64) in SMALL and inst(1, 8, 16 * 161, 3, 1, 64, 0, 64) == D64


def test_instance_bound_and_forced_instances():
    """The 32-pixel tiles where 64-pixel tiles would number fewer than the bound, else the 64-pixel tiles: one 64-pixel tile takes
    the 32-pixel instance, a map of many thousands of tiles the 64-pixel one, and the switch is monotone in between."""
    with options(conv_small=1 << 30, conv_small_fill=1 << 20):
        assert inst(1, 4, 4, 3, 1, 64, 0, 64) == S32
        assert inst(8, 80, 80, 3, 1, 64, 0, 128) == S64
        codes = [inst(1, 8, 8 * t, 3, 1, 64, 0, 64) for t in range(1, 400)]            # t tiles of 64 pixels x one column tile
        flip = codes.index(S64)
        assert codes[:flip] == [S32] * flip and codes[flip:] == [S64] * (len(codes) - flip)
        # ... counted in 64 x 64 tiles: two column tiles halve the pixels at which it flips
        codes2 = [inst(1, 8, 8 * t, 3, 1, 64, 0, 128) for t in range(1, 400)]
        assert codes2.index(S64) + 1 == (flip + 1 + 1) // 2
    for rows, code in ((64, S64), (32, S32)):
        with options(conv_small=1 << 30, conv_small_fill=1 << 20, conv_small_rows=rows):
            assert inst(1, 4, 4, 3, 1, 64, 0, 64) == code and inst(8, 80, 80, 3, 1, 64, 0, 128) == code


def test_ineligible_shapes_keep_their_codes():
    with options(conv_small=1 << 20, conv_small_fill=1 << 20):
        assert inst(2, 20, 20, 3, 1, 64, 0, 64) in SMALL
        assert inst(2, 20, 20, 3, 1, 32, 0, 64) == yv.CONV_IGEMM_64 | ST               # Cin 32
        assert inst(2, 20, 20, 3, 1, 96, 0, 64) == yv.CONV_IGEMM_64 | ST               # Cin 96
        assert inst(2, 20, 20, 3, 1, 64, 0, 56) == yv.CONV_IGEMM_64 | ST               # Cout 56
        assert yv.lib.yv_conv2d_instance(2, 20, 20, 3, 1, 64, 64, 64, 64, 0, yv.EPI_BIAS, 0) == -1      # a two-source 3 x 3
        assert inst(2, 20, 20, 1, 1, 32, 96, 64) == yv.CONV_IGEMM_64 | ST | TWO        # c0 % 64 != 0
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, out_ld=68) == yv.CONV_IGEMM_64         # a misaligned output stride
        assert inst(2, 20, 20, 3, 1, 64, 0, 64, res_ld=68, flags=yv.EPI_RES_BF16) == yv.CONV_IGEMM_64
        assert inst(2, 20, 20, 1, 1, 64, 64, 64) in SMALL                              # two sources on 64-channel boundaries
    with options(conv_small=1 << 20, conv_small_fill=1 << 20, staged_epilogue=0):
        assert inst(2, 20, 20, 3, 1, 64, 0, 64) == yv.CONV_IGEMM_64


def test_ahead_of_splitk():
    shape = (2, 20, 20, 3, 1, 128, 0, 128)                                             # M = 800: what split-K takes with a workspace
    with options(conv_splitk=1):
        assert inst(*shape) == yv.CONV_IGEMM_128 | SK
    with options(conv_splitk=1, conv_small=800, conv_small_fill=1 << 20):
        assert inst(*shape) in SMALL                                                   # inside the range: the small route, no split
        assert inst(2, 20, 21, 3, 1, 128, 0, 128) == yv.CONV_IGEMM_128 | SK            # outside: split-K as before


def test_training_routes_do_not_see_the_option():
    def training():
        a = yv.conv_bnbwd_route(2, 20, 20, 3, 1, 128, 128)
        b = yv.conv_bnbwd_route(1, 20, 20, 1, 1, 256, 128)
        c = yv.conv_dgrad_s2_route(2, 40, 40, 3, 64, 128)
        return [tuple(getattr(r, f) for f in r._fields) if hasattr(r, "_fields") else repr(r) for r in (a, b, c)]

    with options():
        off = training()
    with options(conv_small=1 << 20, conv_small_fill=1 << 20):
        assert training() == off
    with options(conv_small=1 << 20, conv_small_fill=1 << 20, conv_small_rows=32):
        assert training() == off
