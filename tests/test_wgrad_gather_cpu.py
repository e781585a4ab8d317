"""The im2col-free weight gradient of the 3 x 3 convolutions by gathered source addresses (yv_wgrad_conv3_gather), as far as it
goes without a GPU: the kernels' own index function (exported host-only as yv_wgrad_conv3_gather_src; it runs through the
multiply-shift constants the launch computes) against the definition in im2col3_kernel, a pure-torch restatement built on it
against autograd, the route against yv_wgrad_route, the rejected arguments, and YoloTrainer(gather_wgrad=True) through the launch
trace of tests/yolo_trainer_trace.py."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn.functional as F

import yolo_trainer_trace as ytt
import yvhip as yv
from yvhip.yolo_training import Block, YoloTrainer, train_launches

ERR_ARG = -1
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
SMALL_GRIDS = [(1, 1, 1, 1), (1, 2, 2, 2), (2, 7, 5, 2), (2, 6, 10, 2), (3, 5, 4, 1), (1, 64, 1, 2)]
S2_LAYERS = ("model.0", "model.1", "model.3", "model.5", "model.7", "model.16", "model.19")


def r64(n):
    return (n + 63) // 64 * 64


def out_grid(Hin, Win, stride):
    return (Hin - 1) // stride + 1, (Win - 1) // stride + 1


def definition(B, Hin, Win, stride, m, tap):
    """im2col3_kernel's source of (row m, tap): the input pixel index, -1 for a zero."""
    Hout, Wout = out_grid(Hin, Win, stride)
    if m >= B * Hout * Wout:
        return -1
    ox, q = m % Wout, m // Wout
    oy, b = q % Hout, q // Hout
    iy, ix = oy * stride + tap // 3 - 1, ox * stride + tap % 3 - 1
    return (b * Hin + iy) * Win + ix if 0 <= iy < Hin and 0 <= ix < Win else -1


def src(B, Hin, Win, stride, m, tap):
    pixel = C.c_longlong(-7)
    assert yv.lib.yv_wgrad_conv3_gather_src(B, Hin, Win, stride, m, tap, C.byref(pixel)) == 0
    return pixel.value


@pytest.mark.parametrize("B,Hin,Win,stride", SMALL_GRIDS)
def test_index_function_is_the_definition_on_small_grids(B, Hin, Win, stride):
    Hout, Wout = out_grid(Hin, Win, stride)
    T = B * Hout * Wout
    zeros = 0
    for m in range(r64(T)):
        for tap in range(9):
            want = definition(B, Hin, Win, stride, m, tap)
            assert src(B, Hin, Win, stride, m, tap) == want, (m, tap)
            zeros += want < 0
    assert zeros >= 9 * (r64(T) - T) and zeros < 9 * r64(T)
    assert yv.wgrad_conv3_gather_src(B, Hin, Win, stride, 0, 4) == 0 and yv.wgrad_conv3_gather_src(B, Hin, Win, stride, 0, 0) == -1


@pytest.mark.parametrize("Hin", [640, 320, 160, 80, 40])
def test_index_function_on_the_trainers_grids(Hin):
    """16 x 640^2, stride 2, sampled: the first and last 130 tokens (the tail rows included) and both sides of every image boundary."""
    B, stride = 16, 2
    Hout, Wout = out_grid(Hin, Hin, stride)
    T = B * Hout * Wout
    ms = set(range(130)) | set(range(r64(T) - 130, r64(T))) | set(range(T - 130, T))
    for b in range(1, B):
        ms |= {b * Hout * Wout - 1, b * Hout * Wout, b * Hout * Wout - Wout, b * Hout * Wout + Wout - 1}
    for m in sorted(ms):
        for tap in range(9):
            assert src(B, Hin, Hin, stride, m, tap) == definition(B, Hin, Hin, stride, m, tap), (m, tap)


def test_index_function_rejects_bad_arguments():
    pixel = C.c_longlong(0)
    f = yv.lib.yv_wgrad_conv3_gather_src
    assert f(2, 7, 5, 2, 0, 0, C.byref(pixel)) == 0
    for bad in ((0, 7, 5, 2, 0, 0), (2, 0, 5, 2, 0, 0), (2, 7, 0, 2, 0, 0), (2, 7, 5, 3, 0, 0), (2, 7, 5, 0, 0, 0), (2, 7, 5, 2, -1, 0),
                (2, 7, 5, 2, 0, 9), (2, 7, 5, 2, 0, -1)):
        assert f(*bad, C.byref(pixel)) == ERR_ARG, bad
    assert f(2, 7, 5, 2, 0, 0, None) == ERR_ARG
    with pytest.raises(yv.YvError):
        yv.wgrad_conv3_gather_src(2, 7, 5, 3, 0, 0)


@pytest.mark.parametrize("B,Hin,Win,stride", SMALL_GRIDS)
def test_restatement_on_the_index_function_equals_autograd(B, Hin, Win, stride):
    """float64 on integer data: the (r64(T), 9*Cin) operand gathered through the index function, times dz, is autograd's weight
    gradient of F.conv2d(stride, padding=1) exactly."""
    Cin, N = 3, 4
    g = torch.Generator().manual_seed(B * 100 + Hin * 10 + Win)
    Hout, Wout = out_grid(Hin, Win, stride)
    T = B * Hout * Wout
    x = torch.randint(-2, 3, (B, Cin, Hin, Win), generator=g).double()
    dz = torch.randint(-1, 2, (B, N, Hout, Wout), generator=g).double()
    w = torch.zeros(N, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride, 1).backward(dz)
    want = w.grad.permute(0, 2, 3, 1).reshape(N, 9 * Cin)
    pixels = x.permute(0, 2, 3, 1).reshape(B * Hin * Win, Cin)
    col = torch.zeros(r64(T), 9, Cin, dtype=torch.float64)
    for m in range(r64(T)):
        for tap in range(9):
            p = src(B, Hin, Win, stride, m, tap)
            if p >= 0:
                col[m, tap] = pixels[p]
    dzm = torch.zeros(r64(T), N, dtype=torch.float64)
    dzm[:T] = dz.permute(0, 2, 3, 1).reshape(T, N)
    assert torch.equal(dzm.t() @ col.view(r64(T), 9 * Cin), want)
    assert float(want.abs().max()) > 0


def s2_layers(scale):
    return [e for e in train_launches(scale, 80) if isinstance(e, Block) and e.k == 3 and e.stride == 2]


def test_route_is_the_wgrad_route_of_the_im2col_path():
    layers = s2_layers("s")
    assert [e.key for e in layers] == list(S2_LAYERS)
    for e in layers:
        hin = 640 // e.down_in
        T = 16 * (hin // 2) ** 2
        for tile_n in (0, 32, 64, 128):
            for ws in (yv.STREAM_WS_BYTES, 0):
                r, use = yv.wgrad_conv3_gather_route(16, hin, hin, 2, e.cin, e.cout, tile_n, ws_bytes=ws)
                want = yv.wgrad_route(r64(T), e.cout, 9 * e.cin, tile_n, ws_bytes=ws)
                assert isinstance(use, bool)
                for field in yv.WgradRoute._fields:
                    assert getattr(r, field) == getattr(want, field), (e.key, tile_n, ws, field)
    r, _ = yv.wgrad_conv3_gather_route(2, 7, 5, 2, 32, 8)                    # an odd grid: T = 2 * 4 * 3 = 24 -> 64 rows
    assert r == yv.wgrad_route(64, 8, 288, 0)


def test_route_rejects_what_the_launch_rejects():
    out, use = (C.c_int * 5)(), C.c_int(0)
    f = yv.lib.yv_wgrad_conv3_gather_route
    ok = dict(B=2, Hin=8, Win=8, stride=2, Cin=16, N=32, tile_n=0)
    call = lambda o=out, u=C.byref(use), n_cu=256, **kw: f(*dict(ok, **kw).values(), yv.STREAM_WS_BYTES, n_cu, o, u)
    assert call() == 0
    for kw in (dict(stride=3), dict(stride=0), dict(Cin=4), dict(Cin=12), dict(Cin=0), dict(N=12), dict(N=0), dict(tile_n=256),
               dict(tile_n=48), dict(B=0), dict(Hin=0), dict(Win=-1), dict(n_cu=-1), dict(o=None), dict(u=None)):
        assert call(**kw) == ERR_ARG, kw
    with pytest.raises(yv.YvError):
        yv.wgrad_conv3_gather_route(2, 8, 8, 3, 16, 32)


def _launch(dY=P, ldy=32, X=P, ldx=16, B=2, Hin=8, Win=8, stride=2, Cin=16, N=32, dW=P, ldw=144, tile_n=0):
    return yv.lib.yv_wgrad_conv3_gather(dY, ldy, X, ldx, B, Hin, Win, stride, Cin, N, dW, ldw, tile_n, None)


def test_launch_rejects_bad_arguments_on_the_host():
    """No GPU call is made: every case fails validation first (the pointers are host addresses)."""
    for kw in (dict(stride=3), dict(stride=0), dict(Cin=4), dict(Cin=12), dict(ldx=8), dict(ldx=20), dict(dY=P + 8), dict(X=P + 2),
               dict(dW=P + 4), dict(N=36), dict(N=0), dict(tile_n=256), dict(tile_n=48), dict(dY=None), dict(X=None), dict(dW=None),
               dict(ldy=24), dict(ldy=36), dict(ldw=136), dict(ldw=146), dict(B=0), dict(Hin=0), dict(Win=0),
               dict(B=1 << 20, Hin=1 << 12, Win=1 << 12, stride=1)):
        assert _launch(**kw) == ERR_ARG, kw


def test_abi_and_wrappers():
    names = yv.header_symbols()
    for n in ("yv_wgrad_conv3_gather", "yv_wgrad_conv3_gather_route", "yv_wgrad_conv3_gather_src"):
        assert n in names and n in yv._SIGS and n not in yv.MISSING
    assert list(inspect.signature(yv.wgrad_conv3_gather).parameters) == ["dy", "x", "dw", "B", "Hin", "Win", "stride", "tile_n"]
    assert inspect.signature(yv.wgrad_conv3_gather).parameters["tile_n"].default is None


def test_trainer_option_is_off_by_default():
    import utils.trainYolo as ty
    assert inspect.signature(YoloTrainer.__init__).parameters["gather_wgrad"].default is None
    assert inspect.signature(ty.train).parameters["gather_wgrad"].default is None


def _strip(calls):
    """Without the im2col path of the stride-2 blocks and what stands in its place."""
    gone = lambda c: c[0] in ("im2col3", "wgrad_conv3_gather") or (c[0] == "wgrad" and str(c[2][1]).startswith("col")) or \
        (c[0] == "aten.zero_" and str(c[2][0]).startswith("col"))
    return [c for c in calls if not gone(c)]


def _steps(calls):
    starts = [i for i, c in enumerate(calls) if c[0] == "blob_nhwc8"]
    return [calls[a:b] for a, b in zip(starts, starts[1:] + [len(calls)])]


@pytest.mark.parametrize("how", ["argument", "environment"])
def test_trainer_trace_with_the_gather_form(monkeypatch, how):
    """YoloTrainer(gather_wgrad=True) / YV_YOLO_GATHER_WGRAD=1 under the launch-trace harness: per step no im2col3, one
    wgrad_conv3_gather on the side stream for each of the seven stride-2 blocks, and - the im2col path and its stand-in taken
    out of both - the calls of the default fixture in its order.  col shrinks to its 8-element floor."""
    fixture = ytt.load_fixture()["default"]
    if how == "argument":
        monkeypatch.setitem(ytt.CASES, "gather", (2, dict(gather_wgrad=True)))
    else:
        monkeypatch.setitem(ytt.CASES, "gather", (2, dict()))
        monkeypatch.setenv("YV_YOLO_GATHER_WGRAD", "1")
    got = ytt.record_case("gather")
    assert got["allocs"]["col"][0] == [8] and fixture["allocs"]["col"][0] != [8]
    assert {k: v for k, v in got["allocs"].items() if k != "col"} == {k: v for k, v in fixture["allocs"].items() if k != "col"}
    steps = _steps(got["calls"])
    assert len(steps) == 2
    for step in steps:
        names = [c[0] for c in step]
        assert "im2col3" not in names
        gathers = [c for c in step if c[0] == "wgrad_conv3_gather"]
        assert len(gathers) == 7 and all(c[1] == 1 for c in gathers)
        assert sorted(c[2][0] for c in gathers) == sorted("dz." + k for k in S2_LAYERS)
        for c in gathers:
            dz, x, dw, B, hin, win, stride = c[2]
            assert (B, stride) == (ytt.B, 2) and hin == win and len(c) == 3                # tile_n left at its default
            assert x.startswith(("x0", "out"))
    for step in _steps(fixture["calls"]):
        assert [c[0] for c in step].count("im2col3") == 7
    assert _strip(got["calls"]) == _strip(fixture["calls"])
    assert len(got["calls"]) < len(fixture["calls"])


def test_trainer_trace_without_implicit_wgrad_ignores_the_flag(monkeypatch):
    """implicit_wgrad=False is the im2col statement of the trainer: the flag has no effect on it."""
    steps, kw = ytt.CASES["serial_im2col_adamw_ema"]
    monkeypatch.setitem(ytt.CASES, "gather_im2col", (steps, dict(kw, gather_wgrad=True)))
    assert ytt.record_case("gather_im2col") == ytt.load_fixture()["serial_im2col_adamw_ema"]


def test_trainer_trace_with_narrow_tiles_passes_the_tile(monkeypatch):
    monkeypatch.setitem(ytt.CASES, "gather_narrow", (1, dict(gather_wgrad=True, narrow_wgrad=True)))
    calls = ytt.record_case("gather_narrow")["calls"]
    gathers = [c for c in calls if c[0] == "wgrad_conv3_gather"]
    assert len(gathers) == 7 and all(c[3] == {"tile_n": 0} for c in gathers) and "im2col3" not in [c[0] for c in calls]
