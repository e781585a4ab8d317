"""Every MXFP8 linear and convolution route against an exact integer reference (operands, cases and references: mx_exact.py,
whose docstring states the construction; test_mx_exact_cpu.py proves on the CPU that these inputs see a wrong scale block, scale
row, pixel, tap, source, K tail or stale row).

Each case asserts the route it exists for (yv_linear_route(mx=1) / yv_conv2d_mxfp8_instance), then runs every form of its epilogue
family.  Forms without a transcendental are compared with torch.equal - the quantised output of yv_linear_mxfp8_q and of the
convolution's MX map against the CPU quantiser of the exact reference, not against another kernel.  GELU, the `out` of SAVE_PRE,
GELU_BWD and SiLU are compared element by element with the fp64 function of the exact argument, within half a bf16 step plus
twice the measured error of the expression the kernel's source uses (mx_exact.FORM_ERR); the worst |error| / bound of each case
is printed.  Outputs are prefilled with sentinels and carry spare rows and columns that must keep them."""
import pytest
import torch

import mx_exact as mx
from mx_exact import SENT_Q, SENT_S, SENTINEL, bf
from mx_reference import emulate_quant_rows, scale_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XR = mx.EXTRA_ROWS


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module", autouse=True)
def release_the_shared_references():
    """The operands and references shared by this module's cases go when the module is done."""
    yield
    _DEV.clear(); _EXP.clear(); mx._LIN.clear()


def r128(n):
    return (n + 127) // 128 * 128


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not torch.equal(got, exp):
        raise AssertionError(f"{what}: {mx.first_diff(got, exp)}")


def within(got, ref, allow, what):
    """Every element of got (bf16) within mx.act_bound(ref, allow) of ref (f64): one bf16 rounding of a value within `allow`
    (the form's error, a number or a tensor) of the reference.  Returns (the worst |error| / bound, the largest share of `allow`
    an element needs beyond half a bf16 step of its reference - the figure that says how close the FORM comes to its bound)."""
    bound = mx.act_bound(ref, allow)
    err = (got.double() - ref).abs()
    over = err > bound
    assert not bool(over.any()), (what, int(over.sum()), float((err / bound).max()), tuple(over.nonzero()[0].tolist()))
    used = ((err - mx.half_ulp_bf16(ref.abs() + allow)) / (allow + 1e-300)).clamp_min(0)      # (<= 1 where the bound holds)
    return float((err / bound).max()), float(used.max())


# ---------------------------------------------------------------------------------------------------------------- linears
_DEV, _EXP = {}, {}


def lin_dev(yv, shape):
    """Device operands of a shape through yv_quant_mxfp8 (cached): the integers, and the weights / bias times 2^-shift."""
    d = mx.lin_data(shape)
    if shape not in _DEV:
        s = 2.0 ** -d["shift"]
        aq, asc = yv.quant_mxfp8(bf(d["a"]).to(DEV))
        wq, wsc = yv.quant_mxfp8(bf(d["w"]).to(DEV))
        wq_s, wsc_s = yv.quant_mxfp8(bf(d["w"] * s).to(DEV))
        _DEV[shape] = dict(aq=aq, asc=asc, wq=wq, wsc=wsc, wq_s=wq_s, wsc_s=wsc_s, bias=d["bias"].to(DEV), bias_s=(d["bias"] * s).to(DEV))
    return d, _DEV[shape]


def lin_exp(shape, what):
    """References of a shape, computed once and left alone."""
    key = (shape, what)
    if key not in _EXP:
        d = mx.lin_data(shape)
        arg = d["lin"].double() * 2.0 ** -d["shift"]
        E = {k: 2 * v for k, v in mx.FORM_ERR.items()}
        if what == "bf16":
            _EXP[key] = bf(d["lin"])
        elif what == "q":
            _EXP[key] = emulate_quant_rows(bf(d["lin"]).float())
        elif what == "pre":
            _EXP[key] = bf(arg.float())
        elif what == "gelu":
            ref = mx.gelu64(arg)
            _EXP[key] = (ref, E["gelu"])
        elif what == "gelu_bwd":
            dd = bf(arg.float()).double()
            ref = dd * mx.gelu_grad64(d["u"].double())
            _EXP[key] = (ref, dd.abs() * E["gelu_grad"], bf(bf(arg.float()).float() * 0.5)[:, mx.AUX_ZERO_COL])
    return _EXP[key]


def buf(M, N, dtype, fill=SENTINEL, pad=8):
    return torch.full((M + XR, N + pad), fill, dtype=dtype, device=DEV)


def split(out, M, N, live=None):
    """(the written block, everything else) of a (M + XR, N + pad) buffer on the CPU; live: rows a device row count leaves."""
    o = out.cpu()
    live = M if live is None else live
    return o[:live, :N], torch.cat([o[:live, N:].flatten(), o[live:].flatten()])


def run_plain(yv, c, d, dv, shape):
    M, N = d["M"], d["N"]
    out = buf(M, N, torch.bfloat16)
    yv.linear_mxfp8(dv["aq"], dv["asc"], dv["wq"], dv["wsc"], dv["bias"], out)
    got, rest = split(out, M, N)
    same(got, lin_exp(shape, "bf16"), f"{c['name']} bias -> bf16")
    assert bool((rest == SENTINEL).all()), (c["name"], "bias -> bf16 wrote outside (the gap of ldo > N, the spare rows)")
    cnt, mul = mx.M_DEV[shape]
    live = cnt * mul
    m_dev = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    cut = buf(M, N, torch.bfloat16)
    yv.linear_mxfp8(dv["aq"], dv["asc"], dv["wq"], dv["wsc"], dv["bias"], cut, m_dev=m_dev, m_mul=mul)
    got_cut, rest = split(cut, M, N, live)
    same(got_cut, got[:live], f"{c['name']} device row count {live}: rows before the cut")
    assert bool((rest == SENTINEL).all()), (c["name"], "device row count: rows past the cut written")
    # yv_linear_mxfp8_q, no activation.  yv_linear_route rejects YV_EPI_OUT_MXFP8, so these launches assert no route of their own;
    # they take the route of the "bias" form asserted above: mx_linear_route lets the flag in only without an f32 output, it does
    # not enter p9_tile_rows, and it is a run-time branch of the same gemm_p9_kernel<MF, false, 0, MX> / gemm_mx_kernel instance
    if N % 128 == 0:
        qb, sb = lin_exp(shape, "q")
        for lv, kw in ((M, {}), (live, dict(m_dev=m_dev, m_mul=mul))):
            q = buf(M, N, torch.uint8, SENT_Q, 16)
            s = torch.full((N // 128, r128(M) + 128, 4), SENT_S, dtype=torch.uint8, device=DEV)
            yv.linear_mxfp8_q(dv["aq"], dv["asc"], dv["wq"], dv["wsc"], dv["bias"], q, s, **kw)
            gq, rest = split(q, M, N, lv)
            same(gq, qb[:lv], f"{c['name']} MX output bytes ({lv} rows)")
            assert bool((rest == SENT_Q).all()), (c["name"], "MX output bytes outside")
            s = s.cpu()
            same(scale_rows(s, lv), sb[:lv], f"{c['name']} MX output scales ({lv} rows)")
            assert bool((s[:, lv:] == SENT_S).all()), (c["name"], "MX output scales outside")
    out = buf(M, N, torch.bfloat16)
    yv.linear_mxfp8(dv["aq"], dv["asc"], dv["wq_s"], dv["wsc_s"], dv["bias_s"], out, flags=yv.EPI_GELU)
    got, rest = split(out, M, N)
    assert bool((rest == SENTINEL).all()), (c["name"], "GELU wrote outside")
    return {"gelu": within(got, *lin_exp(shape, "gelu"), f"{c['name']} GELU")}


def run_f32(yv, c, d, dv, shape):
    M, N = d["M"], d["N"]
    out = buf(M, N, torch.float32)
    yv.linear_mxfp8(dv["aq"], dv["asc"], dv["wq"], dv["wsc"], dv["bias"], out, flags=yv.EPI_OUT_F32)
    got, rest = split(out, M, N)
    same(got, d["lin"], f"{c['name']} f32 output")
    assert bool((rest == SENTINEL).all()), (c["name"], "f32 output wrote outside")
    want = d["x"] + d["lin"]                                       # integers below 2^24: exact
    out = buf(M, N, torch.float32)
    out[:M, :N] = d["x"].to(DEV)
    yv.linear_mxfp8(dv["aq"], dv["asc"], dv["wq"], dv["wsc"], dv["bias"], out, flags=yv.EPI_RES_F32)
    got, rest = split(out, M, N)
    same(got, want, f"{c['name']} f32 residual read-modify-write")
    assert bool((rest == SENTINEL).all()), (c["name"], "f32 residual wrote outside")
    src = buf(M, N, torch.float32, 0.25)
    src[:M, :N] = d["x"].to(DEV)
    keep = src.clone()
    out = buf(M, N, torch.float32)
    yv.linear_mxfp8_ex(dv["aq"], dv["asc"], dv["wq"], dv["wsc"], dv["bias"], out, flags=yv.EPI_RES_F32, res_f32=src)
    got, rest = split(out, M, N)
    same(got, want, f"{c['name']} res_f32 from another tensor")
    assert bool((rest == SENTINEL).all()) and torch.equal(src, keep), (c["name"], "res_f32: wrote outside / changed the source")
    return {}


def run_pre(yv, c, d, dv, shape):
    M, N = d["M"], d["N"]
    out, pre = buf(M, N, torch.bfloat16), buf(M, N, torch.bfloat16)
    yv.linear_mxfp8_ex(dv["aq"], dv["asc"], dv["wq_s"], dv["wsc_s"], dv["bias_s"], out, flags=yv.EPI_GELU | yv.EPI_SAVE_PRE, aux=pre)
    gp, rest_p = split(pre, M, N)
    got, rest = split(out, M, N)
    same(gp, lin_exp(shape, "pre"), f"{c['name']} the pre tensor of SAVE_PRE")
    assert bool((rest == SENTINEL).all()) and bool((rest_p == SENTINEL).all()), (c["name"], "SAVE_PRE wrote outside")
    return {"save_pre": within(got, *lin_exp(shape, "gelu"), f"{c['name']} the out tensor of SAVE_PRE")}


def run_gbwd(yv, c, d, dv, shape):
    M, N = d["M"], d["N"]
    aux = buf(M, N, torch.bfloat16, 0.25)
    aux[:M, :N] = bf(d["u"]).to(DEV)
    keep = aux.clone()
    out = buf(M, N, torch.bfloat16)
    yv.linear_mxfp8_ex(dv["aq"], dv["asc"], dv["wq_s"], dv["wsc_s"], dv["bias_s"], out, flags=yv.EPI_GELU_BWD, aux=aux)
    got, rest = split(out, M, N)
    ref, allow, zero_col = lin_exp(shape, "gelu_bwd")
    assert bool((rest == SENTINEL).all()) and torch.equal(aux, keep), (c["name"], "GELU_BWD: wrote outside / changed aux")
    same(got[:, mx.AUX_ZERO_COL], zero_col, f"{c['name']} GELU_BWD at aux = 0: bf16(bf16(lin) * 0.5)")
    return {"gelu_bwd": within(got, ref, allow, f"{c['name']} GELU_BWD")}


RUN = {"plain": run_plain, "f32": run_f32, "pre": run_pre, "gbwd": run_gbwd}


@pytest.mark.parametrize("name", [c["name"] for c in mx.lin_cases(__import__("yvhip"))])
def test_linear_exact(yv, name):
    c = next(x for x in mx.lin_cases(yv) if x["name"] == name)
    shape = c["shape"]
    d, dv = lin_dev(yv, shape)
    with mx.options(yv, linear_p8_rows=c["rows"]):
        for form, flags, kw in mx.family_queries(yv, c["fam"], d["N"]):
            assert mx.lin_route(yv, c, flags, n_cu=0, **kw) == c["expect"], (name, form)
        ratios = RUN[c["fam"]](yv, c, d, dv, shape)
    torch.cuda.synchronize()
    for form, (r, used) in ratios.items():
        print(f"\n{name} route {c['expect']}: {form} worst |error| / bound {r:.3f}, form allowance used {used:.3f}")


# ----------------------------------------------------------------------------------------------------------- convolutions
def conv_dev(yv, c, d):
    maps = []
    for x, (ch, up, off, ld) in zip(d["bufs"], c["srcs"]):
        m = yv.mx_map(*x.shape, DEV)
        yv.quant_mxfp8_map(bf(x).to(DEV), m)                       # the whole buffer, every channel
        maps.append(m)
    views = [yv.mx_view(m, off, ch, up) for m, (ch, up, off, ld) in zip(maps, c["srcs"])]
    s = 2.0 ** -d["shift"]
    return dict(maps=maps, views=views, w=yv.quant_conv_weight_mxfp8(bf(d["w"]).to(DEV)), w_s=yv.quant_conv_weight_mxfp8(bf(d["w"] * s).to(DEV)),
                bias=d["bias"].to(DEV), bias_s=(d["bias"] * s).to(DEV), res=bf(d["res"]).to(DEV))


def conv_run(yv, c, dv, kind, mx_out=False, bf16_out=True, silu=False):
    """One launch; returns (out (pixels + XR, ld) or None, MX bytes, MX scales) - flat buffers prefilled with the sentinels."""
    B, H, W, cout = c["B"], c["H"], c["W"], c["cout"]
    npix = B * H * W
    flags = {"f32": yv.EPI_OUT_F32, "bf16": 0, "res": yv.EPI_RES_BF16}[kind] | (yv.EPI_SILU if silu else 0)
    out = q = sc = out_mx = None
    if bf16_out:
        out = torch.full((npix + XR, c["out"][1]), SENTINEL, dtype=torch.float32 if kind == "f32" else torch.bfloat16, device=DEV)
    if mx_out:
        q = torch.full((npix + XR, cout + 64), SENT_Q, dtype=torch.uint8, device=DEV)
        sc = torch.full((npix + XR, (cout + 64) // 32), SENT_S, dtype=torch.uint8, device=DEV)
        out_mx = (q[:npix], sc[:npix])
    wq, ws = dv["w_s"] if silu else dv["w"]
    v = dv["views"]
    yv.conv2d_mxfp8(v[0], v[1] if len(v) > 1 else None, B, H, W, c["k"], c["s"], wq, ws, dv["bias_s"] if silu else dv["bias"],
                    out[:npix] if bf16_out else None, c["out"][0], flags, res=dv["res"] if kind == "res" else None,
                    res_c_off=c["res"][0] if kind == "res" else 0, out_mx=out_mx, outq_c_off=32 if mx_out else 0)
    torch.cuda.synchronize()
    return out, q, sc


def conv_split(c, out, off=None, width=None):
    """(the written view (B, H, W, width), everything else) of a flat output buffer, on the CPU."""
    off = c["out"][0] if off is None else off
    width = c["cout"] if width is None else width
    o = out.cpu()
    npix = c["B"] * c["H"] * c["W"]
    view = o[:npix, off:off + width].reshape(c["B"], c["H"], c["W"], width)
    return view, torch.cat([o[:npix, :off].flatten(), o[:npix, off + width:].flatten(), o[npix:].flatten()])


@pytest.mark.parametrize("name", [c["name"] for c in mx.conv_cases()])
def test_conv_exact(yv, name):
    c = next(x for x in mx.conv_cases() if x["name"] == name)
    d = mx.conv_data(c)
    cout = c["cout"]
    with mx.options(yv):
        assert mx.conv_instance(yv, c) == c["inst"], name
        dv = conv_dev(yv, c, d)
        for kind in ("f32", "bf16", "res"):
            got, rest = conv_split(c, conv_run(yv, c, dv, kind)[0])
            same(got, mx.conv_expected(c, d, kind), f"{name} {kind}")
            assert bool((rest == SENTINEL).all()), (name, kind, "wrote outside its channels / rows")
        exp16 = mx.conv_expected(c, d, "bf16")
        qb, sb = emulate_quant_rows(exp16.float())                 # the CPU quantiser of the exact reference
        for bf16_out in (False, True):
            out, q, sc = conv_run(yv, c, dv, "bf16", mx_out=True, bf16_out=bf16_out)
            what = f"{name} MX output {'next to the bf16 output' if bf16_out else 'alone'}"
            gq, rest = conv_split(c, q, 32, cout)
            same(gq, qb, what + ", bytes")
            assert bool((rest == SENT_Q).all()), (what, "bytes outside the view")
            gs, rest = conv_split(c, sc, 1, cout // 32)
            same(gs, sb, what + ", scales")
            assert bool((rest == SENT_S).all()), (what, "scales outside the view")
            if bf16_out:
                got, rest = conv_split(c, out)
                same(got, exp16, what + ", the bf16 output")
                assert bool((rest == SENTINEL).all()), (what, "bf16 output outside its channels / rows")
        got, rest = conv_split(c, conv_run(yv, c, dv, "bf16", silu=True)[0])
        assert bool((rest == SENTINEL).all()), (name, "SiLU wrote outside")
        arg = d["ref"].double() * 2.0 ** -d["shift"]
        ref = mx.silu64(arg)
        ratio, used = within(got, ref, 2 * mx.FORM_ERR["silu"], f"{name} SiLU")
    print(f"\n{name} instance {c['inst']}: SiLU worst |error| / bound {ratio:.3f}, form allowance used {used:.3f}")
