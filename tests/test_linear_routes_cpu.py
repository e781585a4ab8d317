"""The route of a linear - kernel family, instance, split-K, grid - as yv_linear_route reports it: the function the launch path
calls decides it, so pinning it here (no GPU needed) pins what yv_linear / yv_linear_ex / yv_linear_mxfp8(_ex) launch.  The shipped
options on either side of each threshold of the rule, every option that changes it, and the codes of rejected arguments; all at
256 CUs.  Without a workspace unless a test is about split-K."""
import contextlib

import pytest

import yvhip as yv

SHIPPED = {"linear_variant": 1, "linear_skinny": 256, "linear_splitk": 1, "linear_p8": 3, "linear_p8_rows": 0, "linear_p8_cus": 0,
           "linear_p9_small": 1, "linear_p9_small_fixed": 48, "staged_epilogue": 1}
B, GELU, RES, F32, POS = yv.EPI_BIAS, yv.EPI_GELU, yv.EPI_RES_F32, yv.EPI_OUT_F32, yv.EPI_POSEMB
PRE, GBWD = yv.EPI_SAVE_PRE, yv.EPI_GELU_BWD
SKINNY, IGEMM, DMA, P8, P9, MX = yv.LIN_SKINNY, yv.LIN_IGEMM, yv.LIN_DMA, yv.LIN_P8, yv.LIN_P9, yv.LIN_MX
WS = yv.STREAM_WS_BYTES


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
    """(family, tile rows, tile columns) - with the split when there is one."""
    r = route(M, N, K, flags, **kw)
    return (r.kernel, r.tile_rows, r.tile_cols) + ((r.splitk,) if r.splitk > 1 else ())


def test_options_are_the_shipped_ones_by_default():
    for k, v in SHIPPED.items():
        assert yv.get_option(k) == v, k


def test_ids_are_distinct():
    assert [SKINNY, IGEMM, DMA, P8, P9, MX] == list(range(6))
    assert yv.ROUTE_M_DEV > 1023                                                   # above every YV_EPI_* bit


def test_skinny():
    with options():
        r = route(256, 768, 768)
        assert r == yv.LinearRoute(SKINNY, 64, 16, 0, 0, 0, 0, 1, 1, 4 * 48)
        assert kern(257, 768, 768) == (DMA, 128, 128)
        assert kern(64, 1000, 768, B | F32) == (DMA, 128, 128)                    # N % 16 (1000 = 62.5 x 16)
        assert kern(64, 1008, 768, B | F32) == (SKINNY, 64, 16)
        assert kern(64, 768, 800) == (SKINNY, 64, 16)                             # K % 32 == 0 is enough ...
        assert kern(64, 768, 776) == (IGEMM, 128, 128)                            # ... K % 32 != 0: not even a K step of 64
        assert kern(64, 768, 768, B | GELU | RES) == (SKINNY, 64, 16)
        assert kern(64, 768, 768, B | POS) == (DMA, 128, 128)                     # a flag the skinny kernel does not take
        assert kern(64, 768, 768, B | RES, res_f32=True) == (DMA, 128, 128)       # nothing of yv_linear_ex
        assert kern(64, 768, 768, B, m_dev=True) == (SKINNY, 64, 16)        # a device row count is fine
    with options(linear_skinny=0):
        assert kern(64, 768, 768) == (DMA, 128, 128)
        assert kern(1, 768, 768) == (DMA, 128, 128)
    with options(linear_skinny=64):
        assert kern(64, 768, 768) == (SKINNY, 64, 16)
        assert kern(65, 768, 768) == (DMA, 128, 128)


def test_igemm_tile_widths():
    with options():
        for n, bn in ((16, 16), (32, 32), (64, 64), (20, 32), (36, 64)):
            assert kern(1000, n, 768) == (IGEMM, 128, bn), n
        assert kern(1000, 72, 768) == (DMA, 128, 128)                              # more than 64 columns and whole K steps
        assert kern(1000, 72, 776) == (IGEMM, 128, 128)                            # K % 64 != 0
        assert kern(1000, 768, 96) == (IGEMM, 128, 128)
        assert route(1000, 32, 768).grid == 8 and route(1000, 72, 776).grid == 8
        assert kern(12608, 2304, 776) == (IGEMM, 128, 128)                         # even at a persistent shape
    with options(linear_variant=0):
        assert kern(1000, 768, 768) == (IGEMM, 128, 128)
        assert kern(12608, 2304, 768) == (IGEMM, 128, 128)
        assert kern(64, 768, 768) == (IGEMM, 128, 128)                             # and no skinny kernel


def test_splitk():
    shape = (2304, 768, 6336)                                                      # a weight-gradient shape: 18 x 6 tiles, 99 K steps
    with options(linear_skinny=0):
        assert kern(*shape, B) == (DMA, 128, 128)                                  # no workspace
        r = route(*shape, B, ws_bytes=WS)
        assert (r.kernel, r.tile_rows, r.tile_cols, r.splitk, r.grid) == (DMA, 128, 128, 7, 108 * 7)      # 768 / 108 tiles
        assert kern(*shape, F32, ws_bytes=WS) == (DMA, 128, 128, 7)
        assert kern(*shape, B | GELU, ws_bytes=WS) == (DMA, 128, 128)              # only bias / f32 output
        assert kern(*shape, B | RES, ws_bytes=WS) == (DMA, 128, 128)
        assert kern(*shape, B, ws_bytes=WS, m_dev=True) == (DMA, 128, 128)   # suppressed by a device row count
        # the clamps: 768 / tiles, K steps / 4, 8
        assert kern(256, 128, 6336, ws_bytes=WS) == (DMA, 128, 128, 8)             # 2 tiles, 99 K steps
        assert kern(256, 128, 1024, ws_bytes=WS) == (DMA, 128, 128, 4)             # 16 K steps
        assert kern(256, 128, 512, ws_bytes=WS) == (DMA, 128, 128, 2)
        assert kern(256, 128, 448, ws_bytes=WS) == (DMA, 128, 128)                 # 7 K steps: one slice
        assert kern(6144, 1000, 6336, ws_bytes=WS) == (DMA, 128, 128, 2)           # 384 tiles
        assert kern(6145, 1000, 6336, ws_bytes=WS) == (DMA, 128, 128)              # 392 tiles
        # the workspace bound: S x M x N f32 partials, the split is not shrunk to fit
        assert kern(*shape, B, ws_bytes=7 * 2304 * 768 * 4) == (DMA, 128, 128, 7)
        assert kern(*shape, B, ws_bytes=7 * 2304 * 768 * 4 - 1) == (DMA, 128, 128)
        # not where the free-running kernel's small tiles fill the chip: the trainer's 6,304 x 768 x 768 data gradient
        assert kern(6304, 768, 768, 0, ws_bytes=WS) == (P9, 96, 256)
        assert route(6304, 768, 768, 0, ws_bytes=WS).grid == 198
    with options(linear_skinny=0, linear_p9_small=0):
        r = route(6304, 768, 768, 0, ws_bytes=WS)
        assert (r.kernel, r.tile_rows, r.splitk, r.grid) == (DMA, 128, 2, 600)     # 300 tiles, 12 K steps
    with options(linear_skinny=0, linear_splitk=0):
        assert kern(*shape, B, ws_bytes=WS) == (DMA, 128, 128)
    with options(linear_skinny=0, linear_variant=3):                               # the split overrides a forced variant
        assert kern(*shape, B, ws_bytes=WS) == (DMA, 128, 128, 7)
        assert kern(*shape, B) == (DMA, 256, 256)


def test_persistent_eligibility():
    with options():
        assert kern(2048, 2304, 768) == (P9, 96, 256)                              # 22 x 9 = 198 tiles of 96 rows
        assert kern(2047, 2304, 768) == (DMA, 128, 128)
        assert kern(12608, 2304, 768) == (P9, 160, 256)
        assert kern(12608, 2312, 768) == (DMA, 128, 128)                           # N % 256
        assert kern(12608, 2240, 768) == (DMA, 128, 128)
        assert kern(12608, 4096, 1024) == (P9, 160, 256)
        assert kern(12608, 4352, 1024) == (DMA, 128, 128)                          # N > 4,096
        assert kern(12608, 2304, 64) == (DMA, 128, 128)                            # one K step
        assert kern(12608, 2304, 128) == (P9, 160, 256)
        assert kern(12608, 2304, 768, ldo=2308, flags=B | F32) == (DMA, 128, 128)  # output stride % 8
        assert kern(12608, 2304, 768, B | POS) == (DMA, 128, 128)
        assert kern(12608, 2304, 768, B, m_dev=True) == (P9, 160, 256)
        # the 192-tile test (160-row tiles) and, below it, the 128-tile test (96-row tiles): N = 768 is three tile columns
        assert kern(10081, 768, 768) == (P9, 160, 256)                             # 64 x 3 = 192
        assert kern(10080, 768, 768) == (P9, 160, 256)                             # 63 x 3: the small-tile test lets it through
        assert kern(4033, 768, 768) == (P9, 96, 256)                               # 43 x 3 = 129
        assert kern(4032, 768, 768) == (DMA, 128, 128)                             # 42 x 3 = 126
        assert kern(4097, 768, 768)[0] == P9                                       # 43 x 3 = 129 >= 128
        # 32-bit byte offsets: the f32 view of the output
        assert kern(20000, 4096, 1024, ldo=26848)[0] == DMA
        assert kern(20000, 4096, 1024, ldo=26840)[0] == P9
    with options(linear_p9_small=0):
        assert kern(10081, 768, 768) == (P9, 160, 256)
        assert kern(10080, 768, 768) == (DMA, 128, 128)
        assert kern(2048, 2304, 768) == (DMA, 128, 128)
    with options(staged_epilogue=0):
        assert kern(12608, 2304, 768) == (DMA, 128, 128)
        assert route(12608, 2304, 768).staged == 0


def test_linear_p8_values():
    with options(linear_p8=0):
        assert kern(12608, 2304, 768) == (DMA, 128, 128)
        assert kern(12608, 768, 3072, B | RES) == (DMA, 128, 128)
    with options(linear_p8=1):
        assert kern(12608, 2304, 768) == (P8, 160, 256)
        assert kern(12608, 1536, 768) == (P8, 160, 256)
        assert kern(12608, 1280, 768) == (DMA, 128, 128)                           # N >= 1,536 only
        assert kern(12608, 768, 3072, B | RES) == (DMA, 128, 128)
        assert kern(2047, 2304, 768) == (DMA, 128, 128)
    with options(linear_p8=2):
        assert kern(12608, 1280, 768) == (P8, 256, 256)
        r = route(12608, 768, 3072, B | RES)
        assert (r.kernel, r.tile_rows, r.f32out) == (P8, 160, 1)
        assert kern(6304, 768, 768) == (P8, 128, 256)                              # no tile-count test in front of the 8-phase kernel
        assert kern(12608, 768, 3072, B | RES, res_f32=True) == (DMA, 128, 128)    # the trainer's forms: free-running kernel only
    with options(linear_p8=3):
        assert kern(12608, 1280, 768)[0] == P9


def test_f32_outputs_pick_the_kernel_by_the_parity_of_the_k_tiles():
    with options():
        r = route(12608, 768, 3072, B | RES)                                       # 48 K tiles
        assert (r.kernel, r.tile_rows, r.f32out, r.ext) == (P9, 160, 1, 0)
        r = route(12608, 768, 3008, B | RES)                                       # 47
        assert (r.kernel, r.tile_rows, r.f32out) == (P8, 160, 1)
        r = route(12608, 768, 3008, B | F32)
        assert (r.kernel, r.tile_rows, r.f32out) == (P8, 160, 1)
        assert route(12608, 768, 3008, B).kernel == P9                             # bf16 output: any parity
        # GELU in front of an f32 output: no persistent kernel has it
        assert kern(12608, 768, 3072, B | GELU | F32) == (DMA, 128, 128)
        assert kern(12608, 768, 3072, B | GELU | RES) == (DMA, 128, 128)
        assert kern(12608, 3072, 768, B | GELU) == (P9, 160, 256)


def test_trainer_forms():
    with options():
        # fc1 forward (GELU + saved pre-activation), fc2 data gradient (GELU backward), a separate f32 residual source
        r = route(6304, 3072, 768, B | GELU | PRE, ldaux=3072)
        assert (r.kernel, r.tile_rows, r.ext, r.f32out) == (P9, 160, 1, 0)
        r = route(6304, 3072, 768, GBWD, ldaux=3072)
        assert (r.kernel, r.tile_rows, r.ext, r.f32out) == (P9, 160, 2, 0)
        r = route(12608, 768, 3072, B | RES, res_f32=True)
        assert (r.kernel, r.tile_rows, r.ext, r.f32out) == (P9, 160, 0, 1)
        # ... and where the 128 x 128 kernel takes them: too few tiles (the small tiles have no trainer epilogue; a plain f32
        # residual form does have them), M < 2,048, an odd K / 64
        assert kern(6304, 768, 3072, B | GELU | PRE, ldaux=768) == (DMA, 128, 128)
        assert kern(6304, 768, 3072, GBWD, ldaux=768) == (DMA, 128, 128)
        assert kern(6304, 768, 3072, B | RES, res_f32=True) == (P9, 96, 256)
        assert kern(4032, 768, 3072, B | RES, res_f32=True) == (DMA, 128, 128)
        assert kern(2047, 3072, 768, B | GELU | PRE, ldaux=3072) == (DMA, 128, 128)
        assert kern(2047, 3072, 768, GBWD, ldaux=3072) == (DMA, 128, 128)
        assert kern(2047, 768, 3072, B | RES, res_f32=True) == (DMA, 128, 128)
        assert kern(6304, 3072, 832, B | GELU | PRE, ldaux=3072) == (DMA, 128, 128)
        assert kern(6304, 3072, 832, GBWD, ldaux=3072) == (DMA, 128, 128)
        assert kern(12608, 768, 3008, B | RES, res_f32=True) == (DMA, 128, 128)
        assert kern(64, 3072, 768, GBWD, ldaux=3072) == (DMA, 128, 128)            # never the skinny kernel
    with options(linear_p8=2):
        assert kern(6304, 3072, 768, B | GELU | PRE, ldaux=3072) == (DMA, 128, 128)


BENCH_ROWS = {   # (M, N, K) -> tile height of the free-running kernel, bf16 output (the ViT-B/16 and ViT-L/16 bench shapes)
    (12608, 2304, 768): 160, (12608, 768, 768): 160, (12608, 3072, 768): 160, (12608, 768, 3072): 160,
    (25216, 2304, 768): 224, (25216, 768, 768): 160, (25216, 3072, 768): 256, (25216, 768, 3072): 160,
    (6304, 2304, 768): 256, (6304, 768, 768): 96, (6304, 3072, 768): 160, (6304, 768, 3072): 96,
    (12608, 3072, 1024): 160, (12608, 1024, 1024): 224, (12608, 4096, 1024): 160, (12608, 1024, 4096): 224,
    (25216, 3072, 1024): 256, (25216, 1024, 1024): 224, (25216, 4096, 1024): 160, (25216, 1024, 4096): 224,
    (6304, 3072, 1024): 160, (6304, 1024, 1024): 160, (6304, 4096, 1024): 224, (6304, 1024, 4096): 160,
}


def test_tile_heights_of_the_bench_shapes():
    with options():
        for (M, N, K), rows in BENCH_ROWS.items():
            r = route(M, N, K)
            tiles = -(-M // rows) * (N // 256)
            assert (r.kernel, r.tile_rows, r.grid) == (P9, rows, min(tiles, 256)), (M, N, K, r)
        # f32 residual stream (proj, fc2): at most 192 rows
        assert route(12608, 768, 768, B | RES).tile_rows == 160
        assert route(25216, 768, 3072, B | RES).tile_rows == 160
        assert route(25216, 1024, 4096, B | RES).tile_rows == 160


def test_tile_heights_forced_by_linear_p8_rows():
    for rows in (96, 128, 160, 192, 224, 256):
        with options(linear_p8_rows=rows):
            assert route(12608, 2304, 768).tile_rows == rows
            assert route(12608, 768, 3072, B | RES).tile_rows == rows              # (the f32 instances exist at every height)
            assert route(12608, 3072, 768, B | GELU | PRE, ldaux=3072).tile_rows == {96: 224, 128: 224, 256: 224}.get(rows, rows)
            assert route(12608, 2304, 832).tile_rows == {160: 224, 192: 224}.get(rows, rows)      # odd K / 64: no 160 / 192 rows
    with options(linear_p8_rows=100):
        assert route(12608, 2304, 768).tile_rows == 256                            # a height without an instance
    for rows in (96, 128, 160, 192, 224, 256):
        with options(linear_p8=2, linear_p8_rows=rows):
            assert route(12608, 2304, 768).tile_rows == max(rows, 128)             # 8-phase kernel: from 128 rows
            r = route(12608, 768, 3072, B | RES)
            assert (r.tile_rows, r.f32out) == (min(max(rows, 128), 192), 1)        # f32 epilogue: up to 192


def test_tile_heights_with_fewer_cus():
    with options(linear_p8_cus=128):
        r = route(12608, 2304, 768)
        assert (r.tile_rows, r.grid) == (192, 128)
        assert route(12608, 768, 768).grid == 128
    with options(linear_p8_cus=400):
        assert route(12608, 2304, 768).grid == 256                                 # never more than the device has
    with options():
        assert route(12608, 2304, 768, n_cu=128).tile_rows == 192


FORCED_DMA = {2: (256, 128, 0), 3: (256, 256, 0), 4: (128, 256, 0), 101: (128, 128, 1), 102: (128, 128, 2), 103: (128, 128, 3),
              104: (128, 128, 4), 201: (256, 256, 1), 202: (256, 256, 2), 203: (256, 256, 3), 204: (256, 256, 4)}


@pytest.mark.parametrize("variant", sorted(FORCED_DMA))
def test_forced_lds_dma_variants(variant):
    bm, bn, abl = FORCED_DMA[variant]
    with options(linear_variant=variant):
        for M, N, K in ((12608, 2304, 768), (64, 768, 768), (1000, 1000, 128)):
            r = route(M, N, K)
            assert (r.kernel, r.tile_rows, r.tile_cols, r.abl) == (DMA, bm, bn, abl)
            assert r.grid == -(-M // bm) * -(-N // bn)
        assert kern(1000, 64, 768) == (IGEMM, 128, 64)


def test_forced_persistent_variants():
    with options(linear_variant=9):
        assert kern(12608, 2304, 768) == (P8, 160, 256)
        assert kern(1000, 2304, 768) == (P8, 128, 256)                             # no M >= 2,048 when forced
        assert kern(6304, 768, 768) == (P8, 128, 256)
        assert kern(1000, 2312, 768) == (DMA, 128, 128)                            # the fall-back: not a persistent shape
        assert kern(1000, 2304, 768, B | POS) == (DMA, 128, 128)
        assert kern(12608, 3072, 768, B | GELU | PRE, ldaux=3072) == (DMA, 128, 128)       # trainer forms: not the 8-phase kernel
    with options(linear_variant=11):
        assert kern(12608, 2304, 768) == (P9, 160, 256)
        assert kern(1000, 2304, 768) == (P9, 96, 256)
        assert kern(4032, 768, 768)[0] == P9                                       # no tile-count test when forced
        assert kern(12608, 768, 3008, B | RES)[0] == P8                            # f32 output, odd K / 64
        assert kern(1000, 4352, 768) == (DMA, 128, 128)
        assert kern(1000, 2304, 768, B | GELU | F32) == (DMA, 128, 128)
        assert kern(12608, 3072, 768, B | GELU | PRE, ldaux=3072) == (P9, 160, 256)
    with options(linear_variant=10):                                               # any other value: 128 x 128
        assert kern(12608, 2304, 768) == (DMA, 128, 128)
        assert kern(64, 768, 768) == (DMA, 128, 128)


MX_CASES = [   # test_mx_train_cpu.py::test_linear_mxfp8_instance_rule, with the tile height
    ((6304, 2304, 768, B), (P9, 256)),                                             # ViT-B/16 bench shape, qkv forward
    ((6304, 3072, 768, B | GELU | PRE), (P9, 160)),                                # fc1 forward
    ((6304, 3072, 768, GBWD), (P9, 160)),                                          # fc2 data gradient
    ((6304, 768, 768, B | RES), (MX, 128)),                                        # N = 768 products: 128 x 128 tiles
    ((12608, 768, 3072, B | RES), (P9, 160)),                                      # ... persistent from R = 64
    ((1000, 3072, 768, GBWD), (MX, 128)),                                          # M < 2,048
]


def test_mx_routes():
    with options():
        for (M, N, K, flags), (k, rows) in MX_CASES:
            ext = bool(flags & (PRE | GBWD))
            r = route(M, N, K, flags, mx=True, ldaux=N if ext else 0)
            assert (r.kernel, r.tile_rows, r.mx, r.splitk) == (k, rows, 1, 1), (M, N, K, flags, r)
            assert yv.lib.yv_linear_mxfp8_instance(M, N, K, flags) == int(r.kernel == P9)
        r = route(6304, 3072, 768, B | GELU | PRE, mx=True, ldaux=3072)
        assert (r.ext, r.f32out, r.grid) == (1, 0, 256)
        assert route(6304, 4096, 1024, B | GELU | PRE, mx=True, ldaux=4096).tile_rows == 224     # the ViT-L/16 shapes
        assert route(6304, 3072, 640, B | GELU | PRE, mx=True, ldaux=3072).tile_rows == 224      # odd K / 128
        assert route(12608, 768, 3072, B | RES, mx=True).f32out == 1
        assert route(12608, 768, 3200, B | RES, mx=True).kernel == MX                            # f32 output, odd K / 128
        assert route(12608, 2304, 128, B, mx=True).kernel == MX                                  # one K step
        assert route(12608, 4352, 768, B, mx=True).kernel == MX
        assert route(6304, 768, 768, B, mx=True).grid == 50 * 6
    for rows in (160, 192, 224):
        with options(linear_p8_rows=rows):
            assert route(6304, 3072, 768, B | GELU | PRE, mx=True, ldaux=3072).tile_rows == rows
    with options(linear_p8_rows=128):
        assert route(6304, 2304, 768, B, mx=True).tile_rows == 256                 # no small MX tiles
    with options(linear_p8=2):
        assert route(6304, 2304, 768, B, mx=True).kernel == MX
    with options(linear_variant=3):
        assert route(6304, 2304, 768, B, mx=True).kernel == MX


def test_rejected_arguments_return_the_codes_of_the_launch_path():
    q = yv.lib.yv_linear_route
    out = (yv.C.c_int * 10)()
    ok = dict(M=1000, N=768, K=768, lda=768, ldo=768, flags=B, res=0, ldaux=0, mx=0, ws=0, cu=256)

    def code(**kw):
        a = dict(ok, **kw)
        return q(a["M"], a["N"], a["K"], a["lda"], a["ldo"], a["flags"], a["res"], a["ldaux"], a["mx"], a["ws"], a["cu"], out)

    with options():
        assert code() == 0
        for bad in (dict(M=0), dict(M=-1), dict(N=0), dict(K=0), dict(K=772), dict(lda=772), dict(N=770), dict(ldo=770),
                    dict(flags=B | yv.EPI_SILU), dict(flags=B | yv.EPI_RES_BF16), dict(flags=B | PRE), dict(flags=GBWD),
                    dict(flags=B | GELU | PRE | F32, ldaux=768), dict(flags=GBWD | RES, ldaux=768),
                    dict(flags=GBWD, ldaux=772), dict(flags=GBWD, ldaux=768, K=776), dict(flags=GBWD, ldaux=64, N=64, ldo=64),
                    dict(res=1, K=776), dict(res=1, N=64, ldo=64), dict(cu=-1)):
            assert code(**bad) == -1, bad                                          # YV_ERR_ARG
        assert code(flags=GBWD, ldaux=768) == 0 and code(res=1, flags=B | RES) == 0
        assert code(mx=1) == 0
        for bad in (dict(K=64), dict(K=832), dict(lda=776), dict(N=772), dict(ldo=772), dict(flags=B | POS), dict(flags=PRE, ldaux=768),
                    dict(flags=B | GELU | PRE), dict(flags=GBWD | GELU, ldaux=768), dict(flags=GBWD | F32, ldaux=768),
                    dict(flags=B, ldaux=768), dict(flags=B, res=1), dict(flags=B | 512), dict(ldo=772, flags=B | F32)):
            assert code(mx=1, **bad) == -1, bad
        assert code(cu=0) == (0 if yv.torch.cuda.is_available() else -4)           # YV_ERR_LAUNCH: no device to ask
    with pytest.raises(yv.YvError):
        yv.linear_route(1000, 770, 768, n_cu=256)
    assert q(1000, 768, 768, 768, 768, B, 0, 0, 0, 0, 256, None) == -1


def test_query_leaves_the_options_alone():
    before = {k: yv.get_option(k) for k in SHIPPED}
    with options(linear_variant=3, linear_p8=1, linear_p8_rows=192):
        route(12608, 2304, 768)
    assert {k: yv.get_option(k) for k in SHIPPED} == before
