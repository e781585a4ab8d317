"""yv_conv2d_stats / yv_conv_stats_ws_floats / yv_bn_stats_finish without a GPU: the symbols, the workspace size rule and the
argument checks.  Every return checked here is decided on the host before any HIP call, so the pointers are host addresses that
are never dereferenced."""
import ctypes as C
import os

import pytest

import yvhip as yv

ERR_ARG, ERR_LIMIT, ERR_WORKSPACE = -1, -2, -3
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
NEW = ("yv_conv2d_stats", "yv_conv_stats_ws_floats", "yv_bn_stats_finish")


def stats_call(B=2, H=20, W=20, k=3, s=1, cin=64, cout=64, flags=0, ws_floats=None, in_ptr=P, weight=P, out=P, stats=P, bias=None,
               in_ld=None, out_ld=None):
    """yv_conv2d_stats on dummy pointers; ws_floats None: exactly what yv_conv_stats_ws_floats asks for."""
    v = yv.yv_view(C.c_void_p(in_ptr), in_ld or cin, cin, 0)
    if ws_floats is None:
        ws_floats = yv.conv_stats_ws_floats(B * H * W, cout)
    return yv.lib.yv_conv2d_stats(C.byref(v), B, H, W, k, s, C.c_void_p(weight), C.c_void_p(bias), cout, C.c_void_p(out),
                                  out_ld or cout, flags, C.c_void_p(stats), ws_floats, None, 0, None)


def test_symbols_in_header_and_library():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "yv_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(yv.lib, name), name
    for name in ("conv_stats_ws_floats", "conv_view_stats", "bn_stats_finish"):
        assert callable(getattr(yv, name)), name


@pytest.mark.parametrize("C_", [8, 32, 80, 144])
def test_workspace_floats(C_):
    """Tile partials for every 128-row tile; the fold output is added exactly where there are more than 2048 tiles, holds at
    most 2048 chunks and at least half as many (groups of ceil(tiles / 2048) tiles)."""
    for T in (1, 5, 127, 128, 129, 1122, 102400, 2048 * 128 - 1, 2048 * 128, 2048 * 128 + 1, 266240, 4096 * 128, 4096 * 128 + 1,
              16 * 320 * 320):
        tiles = -(-T // 128)
        got = yv.conv_stats_ws_floats(T, C_)
        assert got >= tiles * 2 * C_, (T, C_)
        if tiles <= 2048:
            assert got == tiles * 2 * C_, (T, C_)
        else:
            group = -(-tiles // 2048)
            chunks = -(-tiles // group)
            assert 1024 <= chunks <= 2048
            assert got == (tiles + chunks) * 2 * C_, (T, C_, got)
    assert yv.conv_stats_ws_floats(0, C_) == 0 and yv.conv_stats_ws_floats(128, 0) == 0


def test_accepts_the_plain_call_up_to_the_workspace_check():
    """The reference point of the rejections below: the same dummy call with one float too few is rejected for the workspace,
    i.e. it passed every argument check."""
    need = yv.conv_stats_ws_floats(2 * 20 * 20, 64)
    assert stats_call(ws_floats=need - 1) == ERR_WORKSPACE
    assert stats_call(ws_floats=0) == ERR_WORKSPACE
    assert stats_call(flags=yv.EPI_BIAS, bias=P, ws_floats=need - 1) == ERR_WORKSPACE
    assert stats_call(B=1, H=512, W=520, k=1, cin=64, cout=80, ws_floats=2080 * 2 * 80) == ERR_WORKSPACE     # no room for the fold


def test_rejects_null_pointers():
    for kw in (dict(in_ptr=None), dict(weight=None), dict(out=None), dict(stats=None)):
        assert stats_call(**kw) == ERR_ARG, kw
    assert yv.lib.yv_conv2d_stats(None, 2, 20, 20, 3, 1, C.c_void_p(P), None, 64, C.c_void_p(P), 64, 0, C.c_void_p(P), 1 << 20, None, 0,
                                  None) == ERR_ARG
    assert stats_call(flags=yv.EPI_BIAS, bias=None) == ERR_ARG          # a bias flag without a bias


@pytest.mark.parametrize("cout", [4, 12, 20, 60, 68])
def test_rejects_output_channels_that_are_no_multiple_of_8(cout):
    assert stats_call(cout=cout, out_ld=72, ws_floats=1 << 20) == ERR_ARG


@pytest.mark.parametrize("flag", ["EPI_SILU", "EPI_GELU", "EPI_RES_F32", "EPI_RES_BF16", "EPI_OUT_F32", "EPI_POSEMB", "EPI_SAVE_PRE",
                                  "EPI_GELU_BWD", 512, 1024, 1 << 30])
def test_rejects_every_flag_but_bias(flag):
    f = getattr(yv, flag) if isinstance(flag, str) else flag        # (512: YV_EPI_OUT_MXFP8, internal; above: no flag at all)
    assert stats_call(flags=f, ws_floats=1 << 20) == ERR_ARG
    assert stats_call(flags=f | yv.EPI_BIAS, bias=P, ws_floats=1 << 20) == ERR_ARG


def test_rejects_what_conv2d_rejects_and_sub_batched_sources():
    assert stats_call(k=5, ws_floats=1 << 20) == ERR_ARG
    assert stats_call(s=3, ws_floats=1 << 20) == ERR_ARG
    assert stats_call(cin=12, ws_floats=1 << 20) == ERR_ARG
    # 40 images of 320 x 320 pixels at a pixel stride of 336 channels: beyond 2 GB, yv_conv2d_ws takes it in sub-batches
    assert stats_call(B=40, H=320, W=320, k=1, cin=64, in_ld=336, ws_floats=1 << 30) == ERR_LIMIT


def test_bn_stats_finish_argument_checks():
    f = yv.lib.yv_bn_stats_finish
    ok = [C.c_void_p(P), 800, 64, 1e-3, 0.03, C.c_void_p(P), C.c_void_p(P), C.c_void_p(P), C.c_void_p(P), None]
    for i in (0, 5, 6):                                                 # stats_ws, mean, rstd
        a = list(ok); a[i] = None
        assert f(*a) == ERR_ARG, i
    for i in (7, 8):                                                    # one running estimate without the other
        a = list(ok); a[i] = None
        assert f(*a) == ERR_ARG, i
    for T, C_ in ((0, 64), (800, 0), (800, 12), (800, 1032)):
        a = list(ok); a[1], a[2] = T, C_
        assert f(*a) == ERR_ARG, (T, C_)
