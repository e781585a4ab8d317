"""The mid-M route step ("linear_mid") as yv_linear_route reports it, and fit_capacity; no GPU, 256 CUs.
Option off (the default): every route of a shape list that covers each step of section 19 equals the table recorded from the commit
before the option existed (tests/golden/linear_routes_parent.json).  Option on: each condition of the step from both sides."""
import contextlib
import json
import os

import pytest

import yvhip as yv
from yvhip.pipeline import fit_capacity

SHIPPED = {"linear_variant": 1, "linear_skinny": 256, "linear_splitk": 1, "linear_p8": 3, "linear_p8_rows": 0, "linear_p8_cus": 0,
           "linear_p9_small": 1, "linear_p9_small_fixed": 48, "staged_epilogue": 1}
B, GELU, RES, F32, POS = yv.EPI_BIAS, yv.EPI_GELU, yv.EPI_RES_F32, yv.EPI_OUT_F32, yv.EPI_POSEMB
PRE, GBWD = yv.EPI_SAVE_PRE, yv.EPI_GELU_BWD
WS = yv.STREAM_WS_BYTES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_routes_parent.json")


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


def route(M, N, K, flags=B, ws_bytes=0, n_cu=256, **kw):
    return yv.linear_route(M, N, K, flags, ws_bytes=ws_bytes, n_cu=n_cu, **kw)


def kern(M, N, K, flags=B, **kw):
    r = route(M, N, K, flags, **kw)
    return (r.kernel, r.tile_rows, r.tile_cols)


def _parent_cases():
    """(options, (M, N, K, flags), keywords) of every shape tests/test_linear_routes_cpu.py asks about, step by step."""
    c = []
    add = lambda opts, M, N, K, flags=B, **kw: c.append((opts, (M, N, K, flags), kw))
    # 1. skinny
    for a in ((256, 768, 768), (257, 768, 768), (64, 1000, 768, B | F32), (64, 1008, 768, B | F32), (64, 768, 800), (64, 768, 776),
              (64, 768, 768, B | GELU | RES), (64, 768, 768, B | POS)):
        add({}, *a)
    add({}, 64, 768, 768, B | RES, res_f32=True)
    add({}, 64, 768, 768, B, m_dev=True)
    for M in (64, 1):
        add(dict(linear_skinny=0), M, 768, 768)
    for M in (64, 65):
        add(dict(linear_skinny=64), M, 768, 768)
    # 2. register-staged
    for n in (16, 32, 64, 20, 36):
        add({}, 1000, n, 768)
    for a in ((1000, 72, 768), (1000, 72, 776), (1000, 768, 96), (12608, 2304, 776)):
        add({}, *a)
    for a in ((1000, 768, 768), (12608, 2304, 768), (64, 768, 768)):
        add(dict(linear_variant=0), *a)
    # 3. split-K
    shape = (2304, 768, 6336)
    s0 = dict(linear_skinny=0)
    add(s0, *shape, B)
    for f in (B, F32, B | GELU, B | RES):
        add(s0, *shape, f, ws_bytes=WS)
    add(s0, *shape, B, ws_bytes=WS, m_dev=True)
    for a in ((256, 128, 6336), (256, 128, 1024), (256, 128, 512), (256, 128, 448), (6144, 1000, 6336), (6145, 1000, 6336)):
        add(s0, *a, ws_bytes=WS)
    add(s0, *shape, B, ws_bytes=7 * 2304 * 768 * 4)
    add(s0, *shape, B, ws_bytes=7 * 2304 * 768 * 4 - 1)
    add(s0, 6304, 768, 768, 0, ws_bytes=WS)
    add(dict(linear_skinny=0, linear_p9_small=0), 6304, 768, 768, 0, ws_bytes=WS)
    add(dict(linear_skinny=0, linear_splitk=0), *shape, B, ws_bytes=WS)
    add(dict(linear_skinny=0, linear_variant=3), *shape, B, ws_bytes=WS)
    add(dict(linear_skinny=0, linear_variant=3), *shape, B)
    # 4. forced LDS-DMA instances
    for v in (2, 3, 4, 101, 102, 103, 104, 201, 202, 203, 204, 10):
        for a in ((12608, 2304, 768), (64, 768, 768), (1000, 1000, 128), (1000, 64, 768)):
            add(dict(linear_variant=v), *a)
    # 5. persistent
    for a in ((2048, 2304, 768), (2047, 2304, 768), (12608, 2304, 768), (12608, 2312, 768), (12608, 2240, 768), (12608, 4096, 1024),
              (12608, 4352, 1024), (12608, 2304, 64), (12608, 2304, 128), (12608, 2304, 768, B | POS), (10081, 768, 768),
              (10080, 768, 768), (4033, 768, 768), (4032, 768, 768), (4097, 768, 768), (12608, 768, 3072, B | RES),
              (12608, 768, 3008, B | RES), (12608, 768, 3008, B | F32), (12608, 768, 3008, B), (12608, 768, 3072, B | GELU | F32),
              (12608, 768, 3072, B | GELU | RES), (12608, 3072, 768, B | GELU), (25216, 3072, 768), (6304, 768, 3072),
              (25216, 1024, 4096, B | RES)):
        add({}, *a)
    add({}, 12608, 2304, 768, B | F32, ldo=2308)
    add({}, 12608, 2304, 768, B, m_dev=True)
    add({}, 20000, 4096, 1024, ldo=26848)
    add({}, 20000, 4096, 1024, ldo=26840)
    for a in ((10081, 768, 768), (10080, 768, 768), (2048, 2304, 768)):
        add(dict(linear_p9_small=0), *a)
    add(dict(staged_epilogue=0), 12608, 2304, 768)
    for p8 in (0, 1, 2, 3):
        for a in ((12608, 2304, 768), (12608, 1536, 768), (12608, 1280, 768), (12608, 768, 3072, B | RES), (2047, 2304, 768),
                  (6304, 768, 768)):
            add(dict(linear_p8=p8), *a)
    add(dict(linear_p8=2), 12608, 768, 3072, B | RES, res_f32=True)
    for a, kw in (((6304, 3072, 768, B | GELU | PRE), dict(ldaux=3072)), ((6304, 3072, 768, GBWD), dict(ldaux=3072)),
                  ((12608, 768, 3072, B | RES), dict(res_f32=True)), ((6304, 768, 3072, B | GELU | PRE), dict(ldaux=768)),
                  ((6304, 768, 3072, B | RES), dict(res_f32=True)), ((4032, 768, 3072, B | RES), dict(res_f32=True)),
                  ((2047, 3072, 768, GBWD), dict(ldaux=3072)), ((6304, 3072, 832, GBWD), dict(ldaux=3072)),
                  ((64, 3072, 768, GBWD), dict(ldaux=3072))):
        add({}, *a, **kw)
    for rows in (96, 128, 160, 192, 224, 256, 100):
        add(dict(linear_p8_rows=rows), 12608, 2304, 768)
        add(dict(linear_p8_rows=rows), 12608, 768, 3072, B | RES)
    add(dict(linear_p8_cus=128), 12608, 2304, 768)
    add({}, 12608, 2304, 768, n_cu=128)
    for v in (9, 11):
        for a in ((12608, 2304, 768), (1000, 2304, 768), (6304, 768, 768), (1000, 2312, 768), (1000, 2304, 768, B | POS),
                  (12608, 768, 3008, B | RES), (1000, 4352, 768), (1000, 2304, 768, B | GELU | F32)):
            add(dict(linear_variant=v), *a)
    # 6. the default, at the rows the mid-M step would take: the classifier's four products at 2 .. 16 crops, engine flags
    for crops in (2, 4, 8, 16):
        M = crops * 197
        for (N, K, f) in ((2304, 768, B), (768, 768, B | RES), (3072, 768, B | GELU), (768, 3072, B | RES)):
            add({}, M, N, K, f, m_dev=True)
    # MXFP8 operands
    for a, kw in (((6304, 2304, 768, B), {}), ((6304, 3072, 768, B | GELU | PRE), dict(ldaux=3072)), ((6304, 768, 768, B | RES), {}),
                  ((12608, 768, 3072, B | RES), {}), ((1000, 3072, 768, GBWD), dict(ldaux=3072)), ((788, 768, 768, B | RES), {})):
        add({}, *a, mx=True, **kw)
    return c


def current_table():
    """[key, route] per case, in order; the key names the case in the golden file."""
    rows = []
    for opts, args, kw in _parent_cases():
        with options(**opts):
            r = route(*args, **kw)
        rows.append([json.dumps([opts, list(args), kw], sort_keys=True), list(r)])
    return rows


def test_option_off_every_route_is_the_parents():
    assert yv.get_option("linear_mid") == 0                                        # the default
    with open(GOLDEN) as f:
        want = json.load(f)
    with options(linear_mid=0):
        got = current_table()
    assert len(got) == len(want) > 200
    kernels = {r[0] for _, r in want}
    assert kernels == {yv.LIN_SKINNY, yv.LIN_IGEMM, yv.LIN_DMA, yv.LIN_P8, yv.LIN_P9, yv.LIN_MX}       # every step is in the list
    for g, w in zip(got, want):
        assert g == w


MID = (yv.LIN_MID, 64, 64) if hasattr(yv, "LIN_MID") else None
DMA128 = (yv.LIN_DMA, 128, 128)


def test_option_on_the_step_from_both_sides():
    assert yv.LIN_MID == 6
    with options(linear_mid=2048):
        # rows: above the skinny kernel's, up to the option
        assert kern(256, 768, 768) == (yv.LIN_SKINNY, 64, 16)
        assert kern(257, 768, 768) == MID
        assert kern(2048, 768, 768) == MID
        assert kern(2049, 768, 768) == DMA128
        assert kern(2049, 2304, 768) == (yv.LIN_P9, 96, 256)
        # columns and depth
        assert kern(788, 64, 768) == (yv.LIN_IGEMM, 128, 64)
        assert kern(788, 128, 768) == MID
        assert kern(788, 80, 768) == DMA128
        assert kern(788, 1000, 768, B | F32) == DMA128
        assert kern(788, 768, 96) == (yv.LIN_IGEMM, 128, 128)
        assert kern(788, 768, 64) == MID
        # the plain family only
        for f in (B, B | GELU, B | RES, B | F32, 0, B | GELU | F32):
            assert kern(788, 768, 768, f) == MID, f
        assert kern(788, 768, 768, B | POS) == DMA128
        assert kern(788, 768, 768, B | RES, res_f32=True) == DMA128
        assert kern(788, 768, 768, B | GELU | PRE, ldaux=768) == DMA128
        assert kern(788, 768, 768, GBWD, ldaux=768) == DMA128
        # a device row count, strides, a registered workspace on a split-K form
        assert kern(788, 768, 768, B, m_dev=True) == MID
        assert kern(788, 768, 768, B, m_dev=False) == MID
        assert kern(788, 768, 768, B, lda=3 * 768, ldo=2 * 768) == MID
        assert kern(788, 768, 3072, B | F32, ws_bytes=0) == MID
        assert kern(788, 768, 3072, B | F32, ws_bytes=WS) == MID
        assert kern(788, 768, 3072, B, ws_bytes=WS) == MID
        # grid = tiles, one workgroup each
        for M, N in ((257, 128), (320, 768), (321, 192), (788, 2304), (2048, 1024), (394, 3072)):
            r = route(M, N, 768)
            assert (r.kernel, r.grid, r.splitk, r.abl, r.mx) == (yv.LIN_MID, -(-M // 64) * (N // 64), 1, 0, 0)
        assert route(788, 768, 768).grid == 156 and route(788, 2304, 768).grid == 468 and route(394, 3072, 768).grid == 336
        # MXFP8 operands: untouched
        assert route(788, 768, 768, B | RES, mx=True).kernel == yv.LIN_MX
    with options(linear_mid=4096, linear_p8=2):                                    # ahead of the persistent rule
        assert kern(3152, 768, 768) == MID
    with options(linear_mid=0, linear_p8=2):
        assert kern(3152, 768, 768) == (yv.LIN_P8, 128, 256)
    with options(linear_mid=0):
        assert route(788, 768, 3072, B | F32, ws_bytes=WS).splitk > 1              # what that form was


@pytest.mark.parametrize("variant", [0, 2, 3, 4, 9, 10, 11, 101, 102, 103, 104, 201, 202, 203, 204])
def test_a_forced_variant_keeps_its_meaning(variant):
    for a in ((788, 768, 768), (788, 2304, 768), (2048, 3072, 768, B | GELU)):
        with options(linear_variant=variant, linear_mid=0):
            want = route(*a)
        with options(linear_variant=variant, linear_mid=2048):
            assert route(*a) == want and want.kernel != yv.LIN_MID


def test_only_where_128_x_128_tiles_leave_the_chip_short():
    """At most 5/8 of a workgroup per CU on the 128 x 128 route (160 tiles on 256 CUs): measured on the ViT-B / ViT-L products,
    profiles/mid_gemm_kernels.txt."""
    with options(linear_mid=4096):
        assert kern(788, 2304, 768) == MID                                         # 7 x 18 = 126: qkv of ViT-B/16 at 4 crops
        assert kern(788, 3072, 768, B | GELU) == DMA128                            # 7 x 24 = 168: fc1
        assert kern(788, 3072, 1024) == DMA128                                     # qkv of ViT-L/16 at 4 crops
        assert kern(1576, 768, 3072, B | RES) == MID                               # 13 x 6 = 78
        assert kern(1576, 2304, 768) == DMA128                                     # 13 x 18
        assert kern(3152, 768, 3072, B | RES) == MID                               # 25 x 6 = 150
        assert kern(3152, 1024, 4096, B | RES) == (yv.LIN_P9, 96, 256)             # 25 x 8 = 200: the persistent rule's
        assert kern(2560, 1024, 1024) == MID and kern(2561, 1024, 1024)[0] != yv.LIN_MID       # 20 x 8 = 160 | 21 x 8
        assert kern(788, 768, 768, n_cu=64) == DMA128                              # 42 tiles against 40
        assert kern(394, 768, 768, n_cu=64) == MID                                 # 24


def test_the_step_starts_above_the_skinny_bound_and_never_below_257_rows():
    """Rule: max(linear_skinny, 256) < M <= linear_mid.  Switching the skinny kernel off gives its rows to the tiled route, as it
    always did (VitEngine(cls_tail=False) relies on that), not to this kernel."""
    with options(linear_mid=2048, linear_skinny=0):
        assert kern(100, 768, 768) == DMA128
        assert kern(256, 768, 768) == DMA128
        assert kern(257, 768, 768) == MID
    with options(linear_mid=2048, linear_skinny=64):
        assert kern(65, 768, 768) == DMA128
        assert kern(257, 768, 768) == MID
    with options(linear_mid=2048, linear_skinny=512):
        assert kern(512, 768, 768) == (yv.LIN_SKINNY, 64, 16)
        assert kern(513, 768, 768) == MID
    with options(linear_mid=256):
        assert kern(257, 768, 768) == DMA128


def test_the_option_is_known_and_unknown_ones_are_not():
    old = yv.get_option("linear_mid")                                              # fails where the option does not exist
    try:
        yv.set_option("linear_mid", 1024)
        assert yv.get_option("linear_mid") == 1024
    finally:
        yv.set_option("linear_mid", old)
    with pytest.raises(yv.YvError):
        yv.get_option("linear_mid_rows")
    with pytest.raises(yv.YvError):
        yv.set_option("linear_midd", 1)


@pytest.mark.parametrize("total,cap,want", [(0, 100, 0), (1, 100, 1), (3, 100, 4), (4, 100, 4), (5, 100, 8), (65, 100, 100),
                                            (100, 100, 100), (7, 4, 4), (2, 100, 2), (64, 100, 64), (33, 3200, 64), (1, 1, 1)])
def test_fit_capacity(total, cap, want):
    assert fit_capacity(total, cap) == want
