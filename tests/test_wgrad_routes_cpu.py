"""The route of a weight gradient - N tile, K tile, tile count, token slices, workgroups - as yv_wgrad_route reports it: the
function wgrad_impl launches from decides it, so pinning it here (no GPU needed) pins what yv_wgrad / yv_wgrad_tiled /
yv_wgrad_conv3(_tiled) launch.  tile_n = 128 is the rule from before the narrow tiles (restated below in Python); tile_n = 0
is the chooser, pinned from both sides of each of its thresholds; and the codes of rejected arguments on dummy pointers."""
import contextlib
import ctypes as C

import pytest

import yvhip as yv
from yvhip.yolo_training import yolo_wgrad_shapes

ERR_ARG = -1
WS = yv.STREAM_WS_BYTES
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
VIT_B16 = [(6336, 2304, 768), (6336, 768, 768), (6336, 3072, 768), (6336, 768, 3072)]     # tools/wgrad_bench.py
NS = (8, 16, 24, 32, 40, 48, 64, 72, 80, 96, 128, 136, 192, 256)


@contextlib.contextmanager
def options(**kw):
    old = {k: yv.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            yv.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def slices_rule(tiles, T, N, K, ws_bytes, cap=128, split=0):
    """wgrad_slices of csrc/gemm.hip, as it stood before the narrow tiles (its constants are unchanged)."""
    S = max((1024 if tiles <= 16 else 512) // tiles, 1)
    S = min(S, T // (512 if tiles <= 16 else 128), cap if tiles <= 16 else 16)
    if tiles > 16 and split > 0:
        S = split
    S = min(S, ws_bytes // (N * K * 4))
    return S if S >= 2 else 1


def present_rule(T, N, K, ws_bytes, **opt):
    tiles = -(-N // 128) * -(-K // 128)
    S = slices_rule(tiles, T, N, K, ws_bytes, **opt) if ws_bytes else 1
    return yv.WgradRoute(128, 128, tiles, S, tiles * S)


def all_shapes():
    out = [(T, N, K) for scale, nc in (("n", 5), ("s", 80), ("m", 80)) for _, T, N, K, _ in yolo_wgrad_shapes(scale, nc, 640, 16)]
    out += [(T, N, K) for scale in "nsm" for _, T, N, K, _ in yolo_wgrad_shapes(scale, 80, 640, 16, implicit=False)]
    return sorted(set(out + VIT_B16))


def test_shape_list_holds_the_layers_the_narrow_tiles_are_for():
    s = {k: (T, N, K) for k, T, N, K, _ in yolo_wgrad_shapes("s", 80, 640, 16, implicit=False)}
    assert s["model.0.conv"] == (16 * 320 * 320, 32, 72)
    assert s["model.1.conv"] == (16 * 160 * 160, 64, 288)
    assert s["model.2.m.0.cv1.conv"] == (16 * 160 * 160, 32, 288)
    assert s["model.4.m.1.cv2.conv"] == (16 * 80 * 80, 64, 576)
    assert s["model.22.cv3.0.2"] == (16 * 80 * 80, 80, 128)
    p = {k: T for k, T, N, K, _ in yolo_wgrad_shapes("s", 80, 640, 16)}
    assert p["model.2.m.0.cv1.conv"] == (16 * 162 * 162 + 63) // 64 * 64 and p["model.1.conv"] == 16 * 160 * 160


@pytest.mark.parametrize("nc", [5, 80])
@pytest.mark.parametrize("scale", ["n", "s", "m", "l", "x"])
def test_launch_list_holds_the_convolutions_of_the_state_dict(scale, nc):
    """The blocks of train_launches are the convolutions of yolo_conv_keys, key for key with the state dict's channel counts.  The
    package defines the scales n, s and m (engines.YOLO_SCALES); for l and x both functions must refuse alike."""
    from yvhip.engines import YOLO_SCALES, yolo_conv_keys
    from yvhip.yolo_training import Block, train_launches
    if scale not in YOLO_SCALES:
        for fn in (yolo_conv_keys, train_launches):
            with pytest.raises(KeyError):
                fn(scale, nc)
        return
    blocks = [e for e in train_launches(scale, nc) if isinstance(e, Block)]
    got = {(e.key + (".conv" if e.bn else ""), e.cin_real, e.cout_real, e.k) for e in blocks}
    assert got == set(yolo_conv_keys(scale, nc)) and len(blocks) == len(got)


def test_tile_128_is_the_present_rule():
    shapes = all_shapes()
    assert len(shapes) > 60
    for T, N, K in shapes:
        for ws in (0, WS, 1 << 20):
            assert yv.wgrad_route(T, N, K, 128, ws_bytes=ws) == present_rule(T, N, K, ws), (T, N, K, ws)
    for opt in ({"wgrad_split": 1}, {"wgrad_split": 3}, {"wgrad_split": 9}, {"wgrad_split_cap": 1}, {"wgrad_split_cap": 7},
                {"wgrad_split_cap": 1, "wgrad_split": 1}):
        rule = {"cap": opt.get("wgrad_split_cap", 128), "split": opt.get("wgrad_split", 0)}
        with options(**opt):
            for T, N, K in shapes:
                assert yv.wgrad_route(T, N, K, 128) == present_rule(T, N, K, WS, **rule), (T, N, K, opt)
    assert yv.get_option("wgrad_split") == 0 and yv.get_option("wgrad_split_cap") == 128
    # both sides of the slice rule's own thresholds, through the route
    assert yv.wgrad_route(1024, 128, 128, 128).slices == 2 and yv.wgrad_route(960, 128, 128, 128).slices == 1
    assert yv.wgrad_route(6336, 512, 512, 128).tiles == 16 and yv.wgrad_route(6336, 512, 512, 128).slices == 12
    assert yv.wgrad_route(6336, 512, 640, 128).tiles == 20 and yv.wgrad_route(6336, 512, 640, 128).slices == 16
    assert yv.wgrad_route(6336, 2304, 768, 128) == yv.WgradRoute(128, 128, 108, 4, 432)


def chosen_tile(N):
    """Fewest padded columns ceil(N / tile) * tile from {32, 64, 128}, ties to the wider tile."""
    return min((128, 64, 32), key=lambda t: (-(-N // t) * t, -t))


def routed_tile(T, N, K, ws, n_cu=256):
    """The rule of tile_n = 0, restated: the column rule, then a 64-wide tile goes back to 128 when it launches fewer workgroups
    than the 128 x 128 tiles and those fit one round of the 2 * n_cu slots (explicit tiles are pinned by the tests around)."""
    t = chosen_tile(N)
    r, wide = yv.wgrad_route(T, N, K, t, ws_bytes=ws), yv.wgrad_route(T, N, K, 128, ws_bytes=ws)
    return 128 if t == 64 and r.workgroups < wide.workgroups <= 2 * (n_cu or 256) else t


def test_chooser_picks_the_fewest_padded_columns_then_keeps_the_workgroups():
    want = {8: 32, 16: 32, 24: 32, 32: 32, 40: 64, 48: 64, 64: 64, 72: 32, 80: 32, 96: 32, 128: 128, 136: 32, 192: 64, 256: 128}
    assert sorted(want) == list(NS)
    seen = set()
    for N in NS:
        assert chosen_tile(N) == want[N]
        for K in (8, 72, 256, 264, 576):
            for T in (64, 1088, 409600):
                for ws in (0, WS):
                    r, r128 = yv.wgrad_route(T, N, K, 0, ws_bytes=ws), yv.wgrad_route(T, N, K, 128, ws_bytes=ws)
                    assert r.tile_n == routed_tile(T, N, K, ws), (T, N, K, ws, r)
                    assert r.tile_n in (want[N], 128) and (want[N] != 32 or r.tile_n == 32)      # only a 64-wide tile goes back
                    seen.add((want[N], r.tile_n))
                    assert r.tile_k == (128 if r.tile_n == 128 else 256)
                    assert r.tiles == -(-N // r.tile_n) * -(-K // r.tile_k)
                    assert r.workgroups == r.tiles * r.slices
                    assert r.slices >= 1 and (r.slices == 1 or r.slices * N * K * 4 <= ws)
                    assert r.slices == (slices_rule(r.tiles, T, N, K, ws) if ws else 1)
                    assert -(-N // r.tile_n) * r.tile_n <= -(-N // 128) * 128
                    if r.tile_n != 128:
                        assert -(-N // r.tile_n) * r.tile_n < -(-N // 128) * 128      # narrow only where it computes fewer columns
                        assert r.tile_n == 32 or r.workgroups >= r128.workgroups or r128.workgroups > 512
                    assert r == yv.wgrad_route(T, N, K, r.tile_n, ws_bytes=ws)            # 0 is one of the explicit tiles
                    if N % 128 == 0:
                        assert r == r128
    assert seen == {(32, 32), (64, 64), (64, 128), (128, 128)}
    for N in range(8, 1032, 8):                                                          # every width: K = 64 is one k tile either way
        r = yv.wgrad_route(4096, N, 64, 0)
        assert r.tile_n == routed_tile(4096, N, 64, WS) and (N % 128 or r.tile_n == 128), (N, r)
        assert chosen_tile(N) != 32 or r.tile_n == 32
    assert yv.wgrad_route(4096, 104, 64, 0).tile_n == 128                               # 128 = 128 = 128 columns: the widest
    assert yv.wgrad_route(4096, 160, 64, 0).tile_n == 32                                # 160 < 192 < 256


def test_chooser_thresholds_of_the_workgroup_rule():
    """Both sides of each threshold of step 2, on the shapes that set it (profiles/wgrad_narrow_layers_column_rule.txt)."""
    t = lambda T, N, K, **kw: yv.wgrad_route(T, N, K, 0, **kw).tile_n
    assert t(409600, 64, 64) == 64 and t(409600, 64, 128) == 64          # one k tile either way: 128 workgroups both
    assert t(409600, 64, 136) == 128 and t(409600, 64, 192) == 128       # 128 against 256 workgroups of 512 slots
    assert t(409600, 64, 288) == 128 and t(102400, 64, 288) == 128       # model.1 of YOLOv8s, model.3 of YOLOv8n: 256 against 384
    assert yv.wgrad_route(409600, 64, 512, 128).workgroups == 512
    assert t(409600, 64, 512) == 128 and t(409600, 64, 520) == 64        # 512 workgroups fit one round, 640 do not
    assert t(107584, 64, 576) == 64 and t(107584, 64, 1152) == 64        # the model.4 bottlenecks, cv2.0.0
    assert t(28224, 64, 576) == 128 and t(7744, 64, 4608) == 128         # 5 x 55 = 275, 36 x 14 = 504 workgroups
    assert t(25600, 64, 64) == 64 and t(6400, 64, 64) == 64
    assert t(409600, 64, 288, n_cu=128) == 64 and t(409600, 64, 288, n_cu=192) == 128     # 384 workgroups against 256 / 384 slots
    assert t(409600, 64, 288, n_cu=0) == t(409600, 64, 288, n_cu=256)
    assert t(409600, 48, 288) == 128 and t(409600, 40, 64) == 64         # the rule is about the tile, not about N = 64
    assert t(409600, 192, 64) == 64 and t(28224, 64, 2304) == 64        # MORE workgroups (3 x 128 against 2 x 128; 9 x 55 against 18 x 16)
    assert yv.wgrad_route(28224, 64, 2304, 64).workgroups == 495 and yv.wgrad_route(28224, 64, 2304, 128).workgroups == 288
    assert t(409600, 64, 288, ws_bytes=0) == 128 and t(409600, 64, 64, ws_bytes=0) == 64  # no split: 2 against 3 workgroups
    for T, N, K in ((107584, 32, 288), (419904, 32, 288), (409600, 32, 144), (419904, 16, 144), (102400, 80, 128), (6400, 8, 64)):
        assert t(T, N, K) == 32                                          # a 32-wide tile stays (256 against 384 workgroups included)
    assert yv.wgrad_route(107584, 32, 288, 0).workgroups == 256 and yv.wgrad_route(107584, 32, 288, 128).workgroups == 384


def test_forced_tiles():
    assert yv.wgrad_route(1088, 64, 576, 64, ws_bytes=0) == yv.WgradRoute(64, 256, 3, 1, 3)
    assert yv.wgrad_route(1088, 64, 576, 32, ws_bytes=0) == yv.WgradRoute(32, 256, 6, 1, 6)
    assert yv.wgrad_route(1088, 64, 576, 64) == yv.WgradRoute(64, 256, 3, 2, 6)           # 1088 // 512 = 2 slices of 8 and 9 tiles
    assert yv.wgrad_route(1088, 256, 64, 32) == yv.WgradRoute(32, 256, 8, 2, 16)          # a narrow tile where 128 would do
    with options(wgrad_split_cap=1):
        assert yv.wgrad_route(1088, 64, 576, 64).slices == 1
    assert yv.wgrad_route(409600, 64, 576, 0, ws_bytes=64 * 576 * 4 * 5).slices == 5       # S stays within the workspace


def test_route_rejects_what_the_launch_rejects():
    out = (C.c_int * 5)()
    f = yv.lib.yv_wgrad_route
    assert f(1088, 64, 576, 0, WS, 256, out) == 0
    for bad in ((1088, 64, 576, 16), (1088, 64, 576, 96), (1088, 64, 576, -32), (1088, 64, 576, 256),
                (1000, 64, 576, 0), (1088, 60, 576, 0), (1088, 64, 572, 0), (0, 64, 576, 0), (1088, 0, 576, 0)):
        assert f(*bad, WS, 256, out) == ERR_ARG, bad
    assert f(1088, 64, 576, 0, WS, 256, None) == ERR_ARG
    with pytest.raises(yv.YvError):
        yv.wgrad_route(1088, 64, 576, 48)


def _wg(dY=P, ldy=64, X=P, ldx=576, T=1088, N=64, K=576, dW=P, ldw=576, tile_n=0):
    return yv.lib.yv_wgrad_tiled(dY, ldy, X, ldx, T, N, K, dW, ldw, tile_n, None)


def _wg3(dY=P, ldy=64, X=P, Cin=64, pitch=10, T=1088, N=64, dW=P, ldw=576, tile_n=0):
    return yv.lib.yv_wgrad_conv3_tiled(dY, ldy, X, Cin, pitch, T, N, dW, ldw, tile_n, None)


@pytest.mark.parametrize("f", [_wg, _wg3])
def test_tiled_entries_reject_bad_arguments(f):
    """No GPU call is made: every case fails validation first."""
    for t in (1, 16, 48, 96, 127, 129, 256, -64):
        assert f(tile_n=t) == ERR_ARG, t                       # tile_n outside {0, 32, 64, 128}
    for t in (0, 32, 64, 128):
        assert f(T=1000, tile_n=t) == ERR_ARG                  # T & 63
        assert f(N=60, tile_n=t) == ERR_ARG                    # N & 7
        assert f(dY=P + 8, tile_n=t) == ERR_ARG                # misaligned bases
        assert f(X=P + 2, tile_n=t) == ERR_ARG
        assert f(dW=P + 4, tile_n=t) == ERR_ARG
        assert f(dY=None, tile_n=t) == ERR_ARG
        assert f(ldy=60, tile_n=t) == ERR_ARG                  # misaligned strides
        assert f(ldw=574, tile_n=t) == ERR_ARG
        assert f(T=0, tile_n=t) == ERR_ARG
    assert _wg(K=572) == ERR_ARG                               # K & 7
    assert _wg(ldx=572) == ERR_ARG
    assert _wg3(Cin=4) == ERR_ARG                              # Cin < 8
    assert _wg3(Cin=0) == ERR_ARG
    assert _wg3(Cin=12) == ERR_ARG                             # Cin & 7
    assert _wg3(pitch=2) == ERR_ARG
    assert _wg3(X=None) == ERR_ARG


def test_header_declares_the_new_entries():
    names = yv.header_symbols()
    for n in ("yv_wgrad_tiled", "yv_wgrad_conv3_tiled", "yv_wgrad_route"):
        assert n in names and n in yv._SIGS and n not in yv.MISSING
