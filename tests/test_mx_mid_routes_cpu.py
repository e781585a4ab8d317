"""The mid-M step of the MXFP8 route ("linear_mx_mid") as yv_linear_route(mx=1) and
yv_linear_mxfp8_q_route report it; no GPU, 256 CUs.
Option at 0 (the default): the routes of the four exact shapes and of the block products of ViT-B/16, ViT-B/8 and ViT-L/16 at
1 .. 32 crops equal the table recorded from the commit before the option existed (tests/golden/mx_mid_routes_parent.json).
Option on: each condition of the step from both sides.  And the exact-integer gate of test_gpu_mx_mid.py sees the two faults a K
split inside a workgroup can have: a lost K group and a wrong exchange."""
import json
import os

import pytest
import torch

import mx_exact as mx
import mx_mid_cases as mc
import yvhip as yv

B, GELU, RES, F32 = yv.EPI_BIAS, yv.EPI_GELU, yv.EPI_RES_F32, yv.EPI_OUT_F32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mx_mid_routes_parent.json")
ON = mc.OPTIONS_ON
MID = (yv.LIN_MX_MID, 64, 64, 1, 1)


def kern(M, N, K, flags=B, n_cu=256, **kw):
    r = yv.linear_route(M, N, K, flags, mx=True, n_cu=n_cu, **kw)
    return (r.kernel, r.tile_rows, r.tile_cols, r.mx, r.splitk)


def qkern(M, N, K, flags=B, n_cu=256, **kw):
    r = yv.linear_mxfp8_q_route(M, N, K, flags, n_cu=n_cu, **kw)
    return (r.kernel, r.tile_rows, r.tile_cols, r.mx, r.splitk)


def parent_queries():
    """(key, M, N, K, flags) of every route the golden table holds."""
    q = [(f"{s}:{f}", *mc.MID_SHAPES[s], f) for s in mc.MID_SHAPES for f in (B, B | GELU, B | F32, B | RES)]
    for name, (D, tok) in mc.MODELS.items():
        for crops in mc.CROPS:
            q += [(f"{name}:{crops}:{p}", crops * tok, n, k, flags) for p, n, k, flags, _ in mc.products(yv, D)]
    return q


def test_constants_and_options_exist():
    assert yv.LIN_MX_MID == 7
    from yvhip import engines
    assert 0 < engines.MX_MID_GEMM_ROWS <= 4096
    assert yv.get_option("linear_mx_mid") == 0                       # shipped: the step does not exist
    fill = yv.get_option("linear_mx_mid_fill")
    with mx.options(yv, linear_mx_mid=123, linear_mx_mid_fill=7):
        assert (yv.get_option("linear_mx_mid"), yv.get_option("linear_mx_mid_fill")) == (123, 7)
    assert (yv.get_option("linear_mx_mid"), yv.get_option("linear_mx_mid_fill")) == (0, fill)


def test_option_off_is_the_parents_route():
    want = json.load(open(GOLDEN))
    queries = parent_queries()
    assert sorted(want) == sorted(k for k, *_ in queries)
    with mx.options(yv, linear_mx_mid=0):
        for key, M, N, K, flags in queries:
            r = yv.linear_route(M, N, K, flags, mx=True, n_cu=256, m_dev=True)
            assert list(r) == want[key], (key, r, want[key])
            assert r.kernel in (yv.LIN_MX, yv.LIN_P9)
    # ... whatever the fill says, and for the _q form
    with mx.options(yv, linear_mx_mid=0, linear_mx_mid_fill=1 << 20):
        for s in mc.MID_SHAPES:
            assert kern(*mc.MID_SHAPES[s]) == (yv.LIN_MX, 128, 128, 1, 1)
        for s in mc.Q_SHAPES:
            assert qkern(*mc.MID_SHAPES[s], B | GELU) == (yv.LIN_MX, 128, 128, 1, 1)


def test_option_on_takes_the_shapes_the_rule_states():
    with mx.options(yv, **ON):
        for s, (M, N, K) in mc.MID_SHAPES.items():
            for flags in (B, B | GELU, B | F32, B | RES, B | GELU | F32, 0):
                assert kern(M, N, K, flags) == MID, (s, flags)
            assert kern(M, N, K, B, m_dev=True) == MID
            assert kern(M, N, K, B, ldo=N + 8, lda=K + 128) == MID
            r = yv.linear_route(M, N, K, B, mx=True, n_cu=256)
            assert r.grid == (M + 63) // 64 * (N // 64)
        assert kern(1, 128, 128) == MID                              # no 256-row floor: the MX route has no skinny kernel
        assert kern(4096, 128, 128) == MID
        for name, (D, tok) in mc.MODELS.items():
            for crops in (1, 2, 4, 5):
                for p, n, k, flags, q in mc.products(yv, D):
                    assert kern(crops * tok, n, k, flags, m_dev=True) == MID, (name, crops, p)


def test_each_condition_excludes():
    LIN_MX = (yv.LIN_MX, 128, 128, 1, 1)
    with mx.options(yv, **ON):
        assert kern(300, 64, 384) == LIN_MX                          # N = 64
        assert kern(300, 128, 384) == MID
        assert kern(300, 96, 384) == LIN_MX and kern(300, 160, 384) == LIN_MX and kern(300, 200, 384) == LIN_MX      # N % 64 != 0
        assert kern(300, 384, 384, B | GELU | yv.EPI_SAVE_PRE, ldaux=384) == LIN_MX       # an aux form
        assert kern(300, 384, 384, yv.EPI_GELU_BWD, ldaux=384) == LIN_MX
        assert kern(300, 384, 384, B | RES, res_f32=True) == LIN_MX                      # a res_f32 source
        assert kern(300, 384, 384, B | RES) == MID
        assert kern(4097, 384, 384) == LIN_MX                                            # M above the option
    with mx.options(yv, linear_mx_mid=299, linear_mx_mid_fill=1 << 20):
        assert kern(300, 384, 384) == LIN_MX and kern(299, 384, 384) == MID
    # the fill: 300 x 384 is 3 x 3 = 9 tiles of 128 x 128; 9 * 8 <= fill * n_cu
    with mx.options(yv, linear_mx_mid=4096, linear_mx_mid_fill=1):
        assert kern(300, 384, 384, n_cu=72) == MID and kern(300, 384, 384, n_cu=71) == LIN_MX
    with mx.options(yv, linear_mx_mid=4096, linear_mx_mid_fill=8):
        assert kern(300, 384, 384, n_cu=9) == MID and kern(300, 384, 384, n_cu=8) == LIN_MX
        assert kern(788, 2304, 768, n_cu=256) == MID                 # 7 x 18 = 126 tiles <= 256
        assert kern(1576, 3072, 768, n_cu=256) == LIN_MX             # 13 x 24 = 312 tiles
    with mx.options(yv, linear_mx_mid=4096, linear_mx_mid_fill=0):
        assert kern(300, 384, 384) == LIN_MX
    # K % 128 != 0 is no MX linear at all
    with mx.options(yv, **ON):
        with pytest.raises(yv.YvError):
            kern(300, 384, 320)


def test_q_route_agrees_with_linear_route():
    shapes = [mc.MID_SHAPES[s] for s in mc.Q_SHAPES] + [(788, 3072, 768), (197, 4096, 1024), (4097, 384, 384), (6304, 3072, 768)]
    for opts in (dict(linear_mx_mid=0), ON, dict(linear_mx_mid=4096, linear_mx_mid_fill=2)):
        with mx.options(yv, **opts):
            for M, N, K in shapes:
                for flags in (B, B | GELU):
                    for m_dev in (False, True):
                        a = yv.linear_route(M, N, K, flags, mx=True, n_cu=256, m_dev=m_dev)
                        b = yv.linear_mxfp8_q_route(M, N, K, flags, n_cu=256, m_dev=m_dev)
                        assert (a.kernel, a.tile_rows, a.tile_cols, a.mx, a.splitk, a.grid) == \
                               (b.kernel, b.tile_rows, b.tile_cols, b.mx, b.splitk, b.grid), (opts, M, N, K, flags)
    with mx.options(yv, **ON):
        assert qkern(300, 384, 384, B | GELU)[0] == yv.LIN_MX_MID
        # what yv_linear_mxfp8_q checks: N % 128 == 0, flags within BIAS | GELU; and yv_linear_route keeps rejecting the flag
        for bad in (lambda: qkern(197, 192, 128), lambda: qkern(300, 384, 384, B | RES), lambda: qkern(300, 384, 384, B | F32),
                    lambda: kern(300, 384, 384, B | 512)):      # (YV_EPI_OUT_MXFP8: internal, the Python layer does not name it)
            with pytest.raises(yv.YvError):
                bad()


@pytest.mark.parametrize("shape", list(mc.MID_SHAPES))
def test_gate_is_sensitive(shape):
    """The split emulation equals the exact reference; every scale fault of mx_exact, a lost K group and a wrong exchange change
    nearly every output."""
    d = mc.lin_data(shape)
    assert (d["M"], d["N"], d["K"]) == mc.MID_SHAPES[shape]
    assert torch.equal(mc.emulate_split(d), d["lin"]) and torch.equal(mx.lin_emulate(d), d["lin"])
    share = lambda out: float((out != d["lin"]).float().mean())
    for fault in mx.LIN_FAULTS:
        if fault in ("stale",):
            continue
        s = share(mx.lin_emulate(d, fault))
        assert s > (0.99 if fault != "drop_last" else 0.9), (shape, fault, s)
    if d["K"] >= 256:
        s = share(mc.emulate_split(d, "lost_group"))
        assert s > 0.99, (shape, "lost_group", s)
    else:
        assert torch.equal(mc.emulate_split(d, "lost_group"), d["lin"])     # one step: group 1 holds nothing
    s = share(mc.emulate_split(d, "wrong_exchange"))
    assert s > 0.95, (shape, "wrong_exchange", s)
