"""gemm_mx_mid_kernel (the "linear_mx_mid" route step) against the exact integer references of mx_exact at
the shapes of mx_mid_cases (one, three, five and eight K steps; ragged last row tiles of 5, 44, 1 and 2 rows).  Every case asserts
its route first.  Forms without a transcendental are compared with torch.equal against the fp32 CPU reference and against the
same call on the 128 x 128 MX route (integer operands: the order of the sums cannot matter); GELU element by element with the fp64
function of the exact argument under the project's bound; the _q form against the CPU quantiser and against linear_mxfp8 +
quant_mxfp8 on the same route.  Outputs are prefilled with sentinels, have a row stride of N + 8 and spare rows that must keep
them; the A operand has a row stride above K."""
import pytest
import torch

import mx_exact as mx
import mx_mid_cases as mc
from mx_exact import SENT_Q, SENT_S, SENTINEL, bf
from mx_reference import emulate_quant_rows, scale_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XR = mx.EXTRA_ROWS
SHAPES = list(mc.MID_SHAPES)


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module", autouse=True)
def release_the_shared_references():
    yield
    _DEV.clear(); _EXP.clear()
    for s in SHAPES:
        mx._LIN.pop(s, None)


def r128(n):
    return (n + 127) // 128 * 128


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not torch.equal(got, exp):
        raise AssertionError(f"{what}: {mx.first_diff(got, exp)}")


_DEV, _EXP = {}, {}


def lin_dev(yv, shape):
    """Device operands of a shape through yv_quant_mxfp8 (cached): A in a buffer of row stride K + 128 (the spare columns hold
    bytes a kernel that ignored the stride would read), the weights, and the weights / bias times 2^-shift."""
    d = mc.lin_data(shape)
    if shape not in _DEV:
        M, K = d["M"], d["K"]
        s = 2.0 ** -d["shift"]
        wide = torch.full((M, K + 128), 0x7E, dtype=torch.uint8, device=DEV)           # 0x7e = 448: loud if read
        dense, asc = yv.quant_mxfp8(bf(d["a"]).to(DEV))
        wide[:, :K] = dense
        aq = wide[:, :K]
        assert aq.stride(0) == K + 128
        wq, wsc = yv.quant_mxfp8(bf(d["w"]).to(DEV))
        wq_s, wsc_s = yv.quant_mxfp8(bf(d["w"] * s).to(DEV))
        _DEV[shape] = dict(aq=aq, asc=asc, wq=wq, wsc=wsc, wq_s=wq_s, wsc_s=wsc_s, bias=d["bias"].to(DEV), bias_s=(d["bias"] * s).to(DEV))
    return d, _DEV[shape]


def lin_exp(shape, what):
    key = (shape, what)
    if key not in _EXP:
        d = mc.lin_data(shape)
        if what == "bf16":
            _EXP[key] = bf(d["lin"])
        elif what == "q":
            _EXP[key] = emulate_quant_rows(bf(d["lin"]).float())
        elif what == "gelu":
            _EXP[key] = mx.gelu64(d["lin"].double() * 2.0 ** -d["shift"])
    return _EXP[key]


def buf(M, N, dtype, fill=SENTINEL, pad=8):
    return torch.full((M + XR, N + pad), fill, dtype=dtype, device=DEV)


def split(out, M, N, live=None):
    o = out.cpu()
    live = M if live is None else live
    return o[:live, :N], torch.cat([o[:live, N:].flatten(), o[live:].flatten()])


def routed(yv, d, flags, mid=True, **kw):
    """The route the next launch takes, asserted: no case silently runs the other kernel."""
    r = yv.linear_route(d["M"], d["N"], d["K"], flags, lda=d["K"] + 128, ldo=d["N"] + 8, mx=True, **kw)
    assert (r.kernel, r.tile_rows, r.tile_cols) == ((yv.LIN_MX_MID, 64, 64) if mid else (yv.LIN_MX, 128, 128)), r


def launch(yv, d, dv, out, flags=0, scaled=False, **kw):
    w, ws, b = (dv["wq_s"], dv["wsc_s"], dv["bias_s"]) if scaled else (dv["wq"], dv["wsc"], dv["bias"])
    yv.linear_mxfp8(dv["aq"], dv["asc"], w, ws, b, out, flags=flags, **kw)


def both_routes(yv):
    """(label, options, mid?) of the new route and of the parent's, in that order."""
    return (("mid", mc.OPTIONS_ON, True), ("128 x 128", dict(linear_mx_mid=0), False))


@pytest.mark.parametrize("shape", SHAPES)
def test_bias_bf16_and_device_row_count(yv, shape):
    d, dv = lin_dev(yv, shape)
    M, N = d["M"], d["N"]
    cnt, mul = mc.M_DEV[shape]
    live = cnt * mul
    assert live < M and live % 64 != 0                              # the cut lies inside a 64-row tile
    m_dev = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    for label, opts, mid in both_routes(yv):
        with mx.options(yv, **opts):
            routed(yv, d, yv.EPI_BIAS, mid)
            out = buf(M, N, torch.bfloat16)
            launch(yv, d, dv, out)
            got, rest = split(out, M, N)
            same(got, lin_exp(shape, "bf16"), f"{shape} {label} bias -> bf16")
            assert bool((rest == SENTINEL).all()), (shape, label, "wrote outside (the gap of ldo > N, the spare rows)")
            routed(yv, d, yv.EPI_BIAS, mid, m_dev=True)
            cut = buf(M, N, torch.bfloat16)
            launch(yv, d, dv, cut, m_dev=m_dev, m_mul=mul)
            got_cut, rest = split(cut, M, N, live)
            same(got_cut, lin_exp(shape, "bf16")[:live], f"{shape} {label} device row count {live}")
            assert bool((rest == SENTINEL).all()), (shape, label, "device row count: rows past the cut written")


@pytest.mark.parametrize("shape", SHAPES)
def test_f32_output_and_residual(yv, shape):
    d, dv = lin_dev(yv, shape)
    M, N = d["M"], d["N"]
    want = d["x"] + d["lin"]                                         # integers below 2^24: exact
    for label, opts, mid in both_routes(yv):
        with mx.options(yv, **opts):
            routed(yv, d, yv.EPI_BIAS | yv.EPI_OUT_F32, mid)
            out = buf(M, N, torch.float32)
            launch(yv, d, dv, out, yv.EPI_OUT_F32)
            got, rest = split(out, M, N)
            same(got, d["lin"], f"{shape} {label} f32 output")
            assert bool((rest == SENTINEL).all()), (shape, label, "f32 output wrote outside")
            routed(yv, d, yv.EPI_BIAS | yv.EPI_RES_F32, mid)
            out = buf(M, N, torch.float32)
            out[:M, :N] = d["x"].to(DEV)
            launch(yv, d, dv, out, yv.EPI_RES_F32)
            got, rest = split(out, M, N)
            same(got, want, f"{shape} {label} f32 residual read-modify-write")
            assert bool((rest == SENTINEL).all()), (shape, label, "f32 residual wrote outside")


@pytest.mark.parametrize("shape", SHAPES)
def test_gelu(yv, shape):
    """Every element against the fp64 GELU of the exact argument: one bf16 rounding of a value within 2 * FORM_ERR["gelu"]."""
    d, dv = lin_dev(yv, shape)
    M, N = d["M"], d["N"]
    ref, allow = lin_exp(shape, "gelu"), 2 * mx.FORM_ERR["gelu"]
    bound = mx.act_bound(ref, allow)
    with mx.options(yv, **mc.OPTIONS_ON):
        for flags, dt in ((yv.EPI_GELU, torch.bfloat16), (yv.EPI_GELU | yv.EPI_OUT_F32, torch.float32)):
            routed(yv, d, yv.EPI_BIAS | flags)
            out = buf(M, N, dt)
            launch(yv, d, dv, out, flags, scaled=True)
            got, rest = split(out, M, N)
            assert bool((rest == SENTINEL).all()), (shape, "GELU wrote outside")
            err = (got.double() - ref).abs()
            print(f"{shape} GELU -> {dt}: worst |error| / bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), (shape, dt, int((err > bound).sum()), float((err / bound).max()))


@pytest.mark.parametrize("shape", mc.Q_SHAPES)
def test_q_form(yv, shape):
    d, dv = lin_dev(yv, shape)
    M, N, K = d["M"], d["N"], d["K"]
    cnt, mul = mc.M_DEV[shape]
    live = cnt * mul
    m_dev = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    qb, sb = lin_exp(shape, "q")

    def q_launch(flags, scaled, lv, **kw):
        w, ws, b = (dv["wq_s"], dv["wsc_s"], dv["bias_s"]) if scaled else (dv["wq"], dv["wsc"], dv["bias"])
        q = buf(M, N, torch.uint8, SENT_Q, 16)
        s = torch.full((N // 128, r128(M) + 128, 4), SENT_S, dtype=torch.uint8, device=DEV)
        yv.linear_mxfp8_q(dv["aq"], dv["asc"], w, ws, b, q, s, flags=flags, **kw)
        gq, rest = split(q, M, N, lv)
        assert bool((rest == SENT_Q).all()), (shape, "MX output bytes outside")
        s = s.cpu()
        assert bool((s[:, lv:] == SENT_S).all()), (shape, "MX output scales of rows past M / of the padding rows written")
        return gq, scale_rows(s, lv)

    with mx.options(yv, **mc.OPTIONS_ON):
        for flags in (yv.EPI_BIAS, yv.EPI_BIAS | yv.EPI_GELU):
            for md in (False, True):
                r = yv.linear_mxfp8_q_route(M, N, K, flags, m_dev=md)
                assert (r.kernel, r.tile_rows, r.tile_cols) == (yv.LIN_MX_MID, 64, 64), r
        # bias only: the CPU quantiser of the exact reference
        for lv, kw in ((M, {}), (live, dict(m_dev=m_dev, m_mul=mul))):
            gq, gs = q_launch(0, False, lv, **kw)
            same(gq, qb[:lv], f"{shape} MX output bytes ({lv} rows)")
            same(gs, sb[:lv], f"{shape} MX output scales ({lv} rows)")
        # bias + GELU: linear_mxfp8 on the same route followed by quant_mxfp8
        routed(yv, d, yv.EPI_BIAS | yv.EPI_GELU)
        h = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        launch(yv, d, dv, h, yv.EPI_GELU, scaled=True)
        q_ref, s_ref = yv.quant_mxfp8(h)
        gq, gs = q_launch(yv.EPI_GELU, True, M)
        same(gq, q_ref.cpu(), f"{shape} GELU MX output bytes against linear_mxfp8 + quant_mxfp8")
        same(gs, scale_rows(s_ref.cpu(), M), f"{shape} GELU MX output scales against linear_mxfp8 + quant_mxfp8")


def test_two_launches_give_equal_bits(yv):
    """Random (non-integer) data: the result does not depend on the launch."""
    g = torch.Generator().manual_seed(38)
    M, N, K = 300, 384, 640
    aq, asc = yv.quant_mxfp8(torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV))
    wq, wsc = yv.quant_mxfp8((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV))
    bias = torch.randn(N, generator=g).to(DEV)
    with mx.options(yv, **mc.OPTIONS_ON):
        for flags, dt in ((0, torch.bfloat16), (yv.EPI_OUT_F32, torch.float32), (yv.EPI_GELU, torch.bfloat16)):
            assert yv.linear_route(M, N, K, yv.EPI_BIAS | flags, mx=True).kernel == yv.LIN_MX_MID
            outs = []
            for _ in range(2):
                o = torch.zeros(M, N, dtype=dt, device=DEV)
                yv.linear_mxfp8(aq, asc, wq, wsc, bias, o, flags=flags)
                outs.append(o.cpu())
            assert torch.equal(*outs), (flags, mx.first_diff(*outs))
            assert bool(outs[0].float().abs().sum() > 0)
        assert yv.linear_mxfp8_q_route(M, N, K, yv.EPI_BIAS | yv.EPI_GELU).kernel == yv.LIN_MX_MID
        qs = []
        for _ in range(2):
            q = torch.zeros(M, N, dtype=torch.uint8, device=DEV)
            s = torch.zeros(N // 128, r128(M), 4, dtype=torch.uint8, device=DEV)
            yv.linear_mxfp8_q(aq, asc, wq, wsc, bias, q, s, flags=yv.EPI_GELU)
            qs.append((q.cpu(), s.cpu()))
        assert torch.equal(qs[0][0], qs[1][0]) and torch.equal(qs[0][1], qs[1][1])
