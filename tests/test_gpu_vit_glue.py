"""The HBM-bound glue kernels of the ViT trainer (csrc/vit_bwd.hip, csrc/train.hip, csrc/vit_misc.hip), each on its own, every
element against an fp64 reference of its operands and a derived worst-case bound (vit_glue_reference.py, gate 1.01), or bit for
bit where the case is exact: the four column-sum kernels and both second stages at their row and column edges and past 128
partial rows, LayerNorm forward and backward at D up to the limit, with strides, a device-side row count, low variance and a
workspace that is not 16-byte aligned, token_reduce, cls_rows, the wrapper head's backward, the loss up to 32 classes and past
256 rows, sgd_step across a second grid-stride trip, and optim_step / ema_update past their grid.  Outputs are pre-filled with a
bf16-representable sentinel: what lies past the live region must still hold it and every live element must have been written;
inputs past `rows` are NaN and must not leak.  test_vit_glue_reference_cpu.py shows on the CPU that an emulation of each kernel
stays inside the gate and that named wrong kernels fall outside.  Each test prints its worst |got - ref| / B; the module prints
the worst per kernel at its end."""
import math

import pytest
import torch

import vit_glue_reference as vg
from vit_glue_reference import GATE, NAN_ROWS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL_ROWS, TAIL_FLOATS = -24576.0, 3, 64                   # bf16-representable; no result of these cases comes near it
NAN = float("nan")
WORST = {}                                                           # kernel -> (ratio, case)


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    yield yvhip
    print("\nworst |got - ref| / bound per kernel over the case list (gate 1.01):")
    for kernel, (r, case) in sorted(WORST.items()):
        print(f"  vit-glue-bound {kernel} {r:.3f} at {case}")


def _note(kernel, r, case):
    print(f"{kernel} {case}: {r:.3f}")
    if r > WORST.get(kernel, (-1.0, None))[0]:
        WORST[kernel] = (r, case)


def _gate(kernel, case, got, ref, bound):
    r, i = vg.worst(got, ref, bound)
    _note(kernel, r, case)
    assert r <= GATE, f"{kernel} {case}: |got - ref| / bound = {r} at flat index {i}"


def _full(shape, fill=SENTINEL, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device=DEV)


def _vec(live, tail=TAIL_FLOATS):
    """device vector of live.numel() + tail sentinels; `live` (or None: sentinels) in front"""
    n = live if isinstance(live, int) else live.numel()
    v = _full(n + tail)
    if not isinstance(live, int):
        v[:n] = live.reshape(-1).to(DEV)
    return v


def _untouched(t):
    return bool((t == SENTINEL).all())


def _written(t):
    return bool(torch.isfinite(t.float()).all()) and not bool((t == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ cast_colsum
def _cast_colsum(yv, x, want_y=True, want_cs=True, start=None, misaligned=False):
    """x (rows, cols) f32 on the CPU -> (y (rows + TAIL_ROWS, cols) bf16, colsum (cols + TAIL_FLOATS)) on the CPU.  NaN rows follow x."""
    rows, cols = x.shape
    off = 1 if misaligned else 0
    buf = _full(off + (rows + NAN_ROWS) * cols, NAN)
    xd = buf[off:off + rows * cols].view(rows, cols)
    xd.copy_(x)
    y = _full((rows + TAIL_ROWS, cols), SENTINEL, torch.bfloat16) if want_y else None
    cs = _vec(cols if start is None else start) if want_cs else None
    nws = yv.colsum_ws_floats(rows, cols)
    ws = _full(nws + TAIL_FLOATS)
    yv.cast_colsum(xd, y, cs, ws, accumulate=start is not None)
    torch.cuda.synchronize()
    assert _untouched(ws[nws:])
    if want_y:
        assert _untouched(y[rows:]) and torch.equal(y[:rows].cpu().view(torch.int16), vg.bf(x).view(torch.int16))     # RNE, bit for bit
    if want_cs:
        assert _untouched(cs[cols:]) and _written(cs[:cols])
    return cs[:cols].cpu() if want_cs else None


@pytest.mark.parametrize("cols", [4, 260, 300, 768, 5, 37])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 47])
def test_cast_colsum(yv, rows, cols):
    """cols % 4 == 0: cast_colsum_vec_kernel + reduce_rows_kernel; else the scalar pair"""
    c = vg.colsum_case("cast", rows, cols)
    _gate("cast_colsum", (rows, cols), _cast_colsum(yv, c["x"]), *vg.colsum_reference(c["x"]))
    ci = vg.colsum_case("cast", rows, cols, exact=True)
    assert torch.equal(_cast_colsum(yv, ci["x"]), ci["x"].sum(0))
    assert torch.equal(_cast_colsum(yv, ci["x"], start=ci["start"]), ci["x"].sum(0) + ci["start"])


@pytest.mark.parametrize("cols", [8, 5])
def test_cast_colsum_130_partial_rows(yv, cols):
    """4131 rows = 130 partial rows: the four-rows-per-trip loop of reduce_rows_kernel (and a tail of 2), 17 trips of the scalar one"""
    rows = 4131
    c = vg.colsum_case("cast", rows, cols)
    _gate("cast_colsum", (rows, cols), _cast_colsum(yv, c["x"]), *vg.colsum_reference(c["x"]))
    _gate("cast_colsum", (rows, cols, "accumulate"), _cast_colsum(yv, c["x"], start=c["start"]), *vg.colsum_reference(c["x"], c["start"]))
    ci = vg.colsum_case("cast", rows, cols, exact=True)
    assert torch.equal(_cast_colsum(yv, ci["x"], start=ci["start"]), ci["x"].sum(0) + ci["start"])


@pytest.mark.parametrize("rows,cols", [(33, 260), (47, 768), (33, 37)])
def test_cast_colsum_options(yv, rows, cols):
    """no y, no column sums, accumulate on a non-zero start, and x one float into its buffer (the scalar cast at cols % 4 == 0)"""
    c, ci = vg.colsum_case("cast", rows, cols), vg.colsum_case("cast", rows, cols, exact=True)
    x = c["x"]
    _gate("cast_colsum", (rows, cols, "no y"), _cast_colsum(yv, x, want_y=False), *vg.colsum_reference(x))
    assert _cast_colsum(yv, x, want_cs=False) is None
    _gate("cast_colsum", (rows, cols, "accumulate"), _cast_colsum(yv, x, start=c["start"]), *vg.colsum_reference(x, c["start"]))
    _gate("cast_colsum", (rows, cols, "x + 4 bytes"), _cast_colsum(yv, x, misaligned=True), *vg.colsum_reference(x))
    assert torch.equal(_cast_colsum(yv, ci["x"], misaligned=True, start=ci["start"]), ci["x"].sum(0) + ci["start"])
    assert torch.equal(_cast_colsum(yv, ci["x"], want_y=False), ci["x"].sum(0))


@pytest.mark.parametrize("rows,cols,misaligned", [(33, 8, False), (47, 260, False), (33, 5, False), (33, 8, True)])
def test_cast_is_rne_bit_for_bit(yv, rows, cols, misaligned):
    """exact ties above even and odd mantissas, their f32 neighbours, +-0, +-inf, overflow to inf, denormals: all three cast paths"""
    _cast_colsum(yv, vg.rne_bits_case(rows, cols), want_cs=False, misaligned=misaligned)


# ------------------------------------------------------------------------------------------------ colsum_bf16
def _colsum_bf16(yv, x, ld, start=None):
    """x (rows, cols) bf16-representable f32 on the CPU, row stride ld >= cols -> colsum (cols) on the CPU; NaN in the gaps and after"""
    rows, cols = x.shape
    buf = _full((rows + NAN_ROWS, ld), NAN, torch.bfloat16)
    buf[:rows, :cols] = x.to(DEV).to(torch.bfloat16)
    cs = _vec(cols if start is None else start)
    nws = yv.colsum_ws_floats(rows, cols)
    ws = _full(nws + TAIL_FLOATS)
    yv.colsum_bf16(buf[:, :cols], cs, ws, rows=rows, accumulate=start is not None)
    torch.cuda.synchronize()
    assert _untouched(ws[nws:]) and _untouched(cs[cols:]) and _written(cs[:cols])
    return cs[:cols].cpu()


@pytest.mark.parametrize("cols,pad", [(8, 0), (8, 8), (264, 0), (264, 8), (1024, 0), (1024, 8), (3072, 0), (3072, 8),      # vector
                                      (8, 4), (264, 4), (300, 0), (300, 4)])                                               # scalar
def test_colsum_bf16(yv, cols, pad):
    for rows in (1, 31, 33, 47, 70):
        c, ci = vg.colsum_case("bf16", rows, cols), vg.colsum_case("bf16", rows, cols, exact=True)
        _gate("colsum_bf16", (rows, cols, cols + pad), _colsum_bf16(yv, c["x"], cols + pad), *vg.colsum_reference(c["x"]))
        assert torch.equal(_colsum_bf16(yv, ci["x"], cols + pad), ci["x"].sum(0))
    _gate("colsum_bf16", (47, cols, cols + pad, "accumulate"), _colsum_bf16(yv, c["x"][:47], cols + pad, c["start"]),
          *vg.colsum_reference(c["x"][:47], c["start"]))
    assert torch.equal(_colsum_bf16(yv, ci["x"], cols + pad, ci["start"]), ci["x"].sum(0) + ci["start"])


@pytest.mark.parametrize("rows,cols", [(9, 1024), (4131, 8)])
def test_colsum_bf16_trainer_shapes(yv, rows, cols):
    """the dfeats call of the trainer (9 rows of 1024), and 130 partial rows behind the vector kernel"""
    c, ci = vg.colsum_case("bf16", rows, cols), vg.colsum_case("bf16", rows, cols, exact=True)
    _gate("colsum_bf16", (rows, cols, cols), _colsum_bf16(yv, c["x"], cols), *vg.colsum_reference(c["x"]))
    assert torch.equal(_colsum_bf16(yv, ci["x"], cols, ci["start"]), ci["x"].sum(0) + ci["start"])


# ------------------------------------------------------------------------------------------------ token_reduce, cls_rows
@pytest.mark.parametrize("R", [1, 3, 33])
def test_token_reduce_exact(yv, R):
    N, D = 5, 100                                                     # N D = 500: two workgroups, the second partly filled
    dx = vg.int_tensor((R, N, D), torch.Generator().manual_seed(R))
    buf = torch.cat([dx, torch.full((1, N, D), NAN)]).to(DEV)
    out = _vec(N * D)
    yv.token_reduce(buf, R, N, D, out)
    torch.cuda.synchronize()
    assert _untouched(out[N * D:]) and torch.equal(out[:N * D].cpu().view(N, D), dx.sum(0))


@pytest.mark.parametrize("R,D", [(1, 100), (3, 100), (33, 100), (3, 300)])
def test_cls_rows_exact(yv, R, D):
    tok = 4
    g = torch.Generator().manual_seed(R + D)
    cls, pos = vg.int_tensor((D,), g), vg.int_tensor((tok + 1, D), g)
    x = _full((R + 1, tok + 1, D))
    yv.cls_rows(cls.to(DEV), pos.to(DEV), R, tok, D, x)
    torch.cuda.synchronize()
    x = x.cpu()
    assert torch.equal(x[:R, 0], (cls + pos[0]).expand(R, D))
    assert _untouched(x[:R, 1:]) and _untouched(x[R:])               # the patch rows and the next crop are not touched


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def _layernorm(yv, c, count=None, rows_per_count=1):
    D, rows = c["D"], c["rows"]
    y = _full((rows + TAIL_ROWS, c["ldy"]), SENTINEL, torch.bfloat16)
    cd = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    yv.layernorm(c["xbuf"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV), y, rows, D, c["ldx"], c["ldy"], eps=vg.LN_EPS, count_dev=cd,
                 rows_per_count=rows_per_count)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("case", vg.LN_FWD_CASES, ids=str)
def test_layernorm_fwd(yv, case):
    c = vg.ln_case(*case)
    D, rows = c["D"], c["rows"]
    y = _layernorm(yv, c)
    assert _untouched(y[rows:]) and _untouched(y[:rows, D:]) and _written(y[:rows, :D])
    _gate("layernorm", case, y[:rows, :D].float(), *vg.ln_fwd_reference(c["x"], c["gamma"], c["beta"]))


@pytest.mark.parametrize("count,live", [(3, 21), (100, 70)])
def test_layernorm_fwd_device_row_count(yv, count, live):
    """rows at run time = min(rows, count_dev[0] * rows_per_count): below `rows` (rows 21.. keep the sentinel) and above it"""
    case = (260, 70, "plain")
    c = vg.ln_case(*case)
    y = _layernorm(yv, c, count, 7)
    assert _untouched(y[live:]) and _written(y[:live])
    ref, bound = vg.ln_fwd_reference(c["x"], c["gamma"], c["beta"])
    _gate("layernorm", (*case, f"count {count}"), y[:live].float(), ref[:live], bound[:live])


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _layernorm_bwd(yv, c, ws_offset=0):
    """-> dx (rows + TAIL_ROWS, ldx), dgamma, dbeta (D) on the CPU.  dbeta, a pad, dgamma and 2 D guard floats share one allocation
    (dbeta first): a second stage that ignores out2 / split then writes inside it and is caught by the sentinel."""
    D, rows, ldx = c["D"], c["rows"], c["ldx"]
    dx = _full((rows + TAIL_ROWS, ldx))
    dx[:rows, :D] = c["dx0"].to(DEV)
    pad = 64
    grads = _full(D + pad + D + 2 * D)
    dbe, dga = grads[:D], grads[D + pad:2 * D + pad]
    nws = int(yv.lib.yv_layernorm_bwd_ws_floats(rows, D))
    wsbuf = _full(ws_offset + nws + TAIL_FLOATS)
    yv.layernorm_bwd(c["xbuf"].to(DEV), ldx, c["gamma"].to(DEV), c["dybuf"].to(DEV), c["ldy"], rows, D, dx, ldx, dga, dbe, wsbuf[ws_offset:],
                     eps=vg.LN_EPS)
    torch.cuda.synchronize()
    assert _untouched(wsbuf[ws_offset + nws:]) and _untouched(wsbuf[:ws_offset])
    assert _untouched(grads[D:D + pad]) and _untouched(grads[2 * D + pad:]), "dgamma / dbeta written outside their D floats"
    assert _written(dga) and _written(dbe)
    assert _untouched(dx[rows:]) and _untouched(dx[:rows, D:]) and bool(torch.isfinite(dx[:rows, :D]).all())
    return dx.cpu(), dga.cpu(), dbe.cpu()


def _check_ln_bwd(yv, case, ws_offset=0, tag=()):
    c = vg.ln_case(*case)
    D, rows = c["D"], c["rows"]
    dx, dga, dbe = _layernorm_bwd(yv, c, ws_offset)
    ref = vg.ln_bwd_reference(c["x"], c["gamma"], c["dy"], c["dx0"])
    _gate("layernorm_bwd dx", (*case, *tag), dx[:rows, :D], ref["dx"], ref["b_dx"])          # dx0 + LN' itself, in fp64
    _gate("layernorm_bwd dgamma", (*case, *tag), dga, ref["dgamma"], ref["b_dgamma"])
    _gate("layernorm_bwd dbeta", (*case, *tag), dbe, ref["dbeta"], ref["b_dbeta"])


@pytest.mark.parametrize("case", vg.LN_BWD_CASES, ids=str)
def test_layernorm_bwd(yv, case):
    _check_ln_bwd(yv, case)


@pytest.mark.parametrize("case", [(260, 9, "plain"), (128, 1037, "plain")], ids=str)
def test_layernorm_bwd_workspace_not_16_byte_aligned(yv, case):
    """the workspace one float into its buffer: launch_reduce_rows takes reduce_rows_scalar_kernel, which must split the 2 D
    columns into dgamma and dbeta as reduce_rows_kernel does"""
    _check_ln_bwd(yv, case, ws_offset=1, tag=("ws + 4 bytes",))


@pytest.mark.parametrize("D,rows,ws_offset", [(260, 9, 0), (128, 1037, 0), (260, 9, 1)])
def test_layernorm_bwd_dbeta_exact(yv, D, rows, ws_offset):
    """dbeta is a plain column sum of dy: integers make it exact"""
    c = dict(vg.ln_case(D, rows, "plain"))
    dy = vg.int_tensor((rows, D), torch.Generator().manual_seed(D + rows))
    c["dybuf"] = vg.bf(torch.cat([dy, torch.full((NAN_ROWS, D), NAN)]))
    assert torch.equal(_layernorm_bwd(yv, c, ws_offset)[2], dy.sum(0))


# ------------------------------------------------------------------------------------------------ wrapper-head backward
@pytest.mark.parametrize("case", vg.HEAD_CASES, ids=str)
def test_head_bwd(yv, case):
    c = vg.head_case(*case)                                           # asserts the ReLU margin
    R, nc, ldf, ldd = case
    H, F = vg.HB_HID, vg.HB_FEAT
    feats = torch.cat([c["feats"], torch.full((NAN_ROWS, ldf), NAN)]).to(DEV)
    dw1, db1, dw2, db2 = _vec(H * F), _vec(H), _vec(nc * H), _vec(nc)
    dfe = _full((R + TAIL_ROWS, ldd), SENTINEL, torch.bfloat16)
    ws = _vec(2 * R * H)
    yv.head_bwd(feats, c["w1"].t().contiguous().to(DEV), c["b1"].to(DEV), c["w2"].to(DEV), c["dl"].to(DEV), R, nc,
                dw1, db1, dw2, db2, dfe, ws)
    torch.cuda.synchronize()
    ref = c["ref"]
    for name, buf, n in (("dw1", dw1, H * F), ("db1", db1, H), ("dw2", dw2, nc * H), ("db2", db2, nc)):
        assert _untouched(buf[n:]) and _written(buf[:n]), name
        _gate("head_bwd " + name, case, buf[:n].cpu().view(ref[name].shape), ref[name], ref["b_" + name])
    assert _untouched(ws[2 * R * H:]) and _untouched(dfe[R:]) and _written(dfe[:R])
    dfe = dfe.cpu().float()
    assert bool((dfe[:R, F:] == 0).all())                             # the padding columns are exactly 0
    _gate("head_bwd dfeats", case, dfe[:R, :F], ref["dfeats"], ref["b_dfeats"])


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("w_ls,w_fo", vg.LOSS_WEIGHTS)
@pytest.mark.parametrize("B,nc", vg.LOSS_SHAPES)
def test_loss_fwd_bwd(yv, B, nc, w_ls, w_fo):
    c = vg.loss_case(B, nc, w_ls, w_fo)
    logits = torch.cat([c["logits"], torch.full((NAN_ROWS, nc), NAN)]).to(DEV)
    labels = torch.cat([c["labels"], torch.full((NAN_ROWS,), 77, dtype=torch.int32)]).to(DEV)
    loss, grad = _vec(1), _vec(B * nc)
    yv.check(yv.lib.yv_loss_fwd_bwd(yv._p(logits), yv._p(labels), B, nc, w_ls, w_fo, yv._p(loss), yv._p(grad), yv._st()), "yv_loss_fwd_bwd")
    torch.cuda.synchronize()
    assert _untouched(loss[1:]) and _untouched(grad[B * nc:]) and _written(loss[:1]) and _written(grad[:B * nc])
    ref = c["ref"]
    w = f"w=({w_ls:.3f}, {w_fo:.3f})"
    _gate("loss_fwd_bwd loss", (B, nc, w), loss[:1].cpu(), ref["loss"].reshape(1), ref["b_loss"].reshape(1))
    _gate("loss_fwd_bwd grad", (B, nc, w), grad[:B * nc].cpu().view(B, nc), ref["grad"], ref["b_grad"])


def test_loss_fwd_bwd_wrapper_defaults(yv):
    """the Python entry point and its default weights on the same case"""
    c = vg.loss_case(257, 5, *vg.LOSS_WEIGHTS[0])
    loss, grad = yv.loss_fwd_bwd(c["logits"].to(DEV), c["labels"].to(DEV))
    torch.cuda.synchronize()
    _gate("loss_fwd_bwd grad", (257, 5, "defaults"), grad.cpu(), c["ref"]["grad"], c["ref"]["b_grad"])
    _gate("loss_fwd_bwd loss", (257, 5, "defaults"), loss.cpu(), c["ref"]["loss"].reshape(1), c["ref"]["b_loss"].reshape(1))


# ------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("n", vg.SGD_NS)
def test_sgd_step_bit_exact_edges(yv, n):
    """two steps: first (m pre-filled with NaN: it must not be read; grad_scale 1/8), then with momentum (grad_scale 1/3); the bf16
    mirror equals bf16 of the new p, tail included; nothing past n is written"""
    g = torch.Generator().manual_seed(n % 1000)
    p0, g1, g2 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01, torch.randn(n, generator=g) * 0.01
    pad = 8
    p, m = _vec(p0, pad), _vec(torch.full((n,), NAN), pad)
    mirror = _full(n + pad, SENTINEL, torch.bfloat16)
    gd = lambda t: torch.cat([t, torch.full((pad,), NAN)]).to(DEV)
    p1, m1, b1 = vg.sgd_reference(p0, g1, None, 1e-4, 0.125, True)
    yv.sgd_step(p[:n], gd(g1)[:n], m[:n], 1e-4, first=True, grad_scale=0.125, mirror=mirror[:n])
    torch.cuda.synchronize()
    for got, ref in ((p, p1), (m, m1), (mirror, b1)):
        assert _untouched(got[n:]) and torch.equal(got[:n].cpu(), ref)
    p2, m2, b2 = vg.sgd_reference(p1, g2, m1, 9.75528e-5, 1.0 / 3.0, False)
    yv.sgd_step(p[:n], gd(g2)[:n], m[:n], 9.75528e-5, first=False, grad_scale=1.0 / 3.0, mirror=mirror[:n])
    torch.cuda.synchronize()
    for got, ref in ((p, p2), (m, m2), (mirror, b2)):
        assert _untouched(got[n:]) and torch.equal(got[:n].cpu(), ref)


def test_sgd_step_without_mirror(yv):
    n = 4096 + 3
    g = torch.Generator().manual_seed(7)
    p0, g1 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    p, m = _vec(p0, 8), _vec(torch.zeros(n), 8)
    yv.sgd_step(p[:n], g1.to(DEV), m[:n], 1e-4, first=True)
    torch.cuda.synchronize()
    p1, m1, _ = vg.sgd_reference(p0, g1, None, 1e-4, 1.0, True)
    assert torch.equal(p[:n].cpu(), p1) and torch.equal(m[:n].cpu(), m1) and _untouched(p[n:]) and _untouched(m[n:])


# ------------------------------------------------------------------------------------------------ optim_step, ema_update
@pytest.mark.parametrize("kind", ["sgd_nesterov", "adamw"])
def test_optimisers_match_torch_past_the_grid(yv, kind):
    """test_gpu_yolo_train.py::test_optimisers_match_torch at n = 4096 * 256 + 3: a second trip of the grid-stride loops of
    optim_kernel and axpby_kernel (4096 workgroups) with a ragged end.  Tolerance from that test's docstring: 1e-5 (torch's
    vectorised CPU kernels contract p + alpha * g into an FMA; measured 3e-6 there)."""
    g = torch.Generator().manual_seed(4)
    n, pad = 4096 * 256 + 3, 8
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.5 + i) for i in range(4)]
    lrs = [1e-3, 2e-3, 5e-4, 1e-3]
    ref = torch.nn.Parameter(p0.clone())
    if kind == "adamw":
        opt = torch.optim.AdamW([ref], lr=lrs[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
        code, b1, wd = yv.OPT_ADAMW, 0.9, 5e-4
    else:
        opt = torch.optim.SGD([ref], lr=lrs[0], momentum=0.937, nesterov=True, weight_decay=5e-4)
        code, b1, wd = yv.OPT_SGD_NESTEROV, 0.937, 5e-4
    p, m, v, ema = _vec(p0, pad), _vec(torch.zeros(n), pad), _vec(torch.zeros(n), pad), _vec(p0, pad)
    mirror = _full(n + pad, SENTINEL, torch.bfloat16)
    ema_ref = p0.clone()
    for t, (gr, lr) in enumerate(zip(grads, lrs), start=1):
        for grp in opt.param_groups:
            grp["lr"] = lr
        ref.grad = gr.clone()
        opt.step()
        yv.optim_step(code, p[:n], gr.to(DEV), m[:n], v[:n], lr, t, beta1=b1, weight_decay=wd, mirror=mirror[:n])
        d = 0.9999 * (1 - math.exp(-t / 2000))
        ema_ref.mul_(d).add_((1 - d) * ref.detach())
        yv.ema_update(ema[:n], p[:n], d)
    torch.cuda.synchronize()
    for buf in (p, m, v, ema, mirror):
        assert _untouched(buf[n:])
    err = float(((p[:n].cpu() - ref.detach()).abs() / (ref.detach().abs() + 1e-3)).max())
    print(f"optim_step {kind} n={n}: max relative difference {err:.2e}")
    assert err < 1e-5, err
    assert torch.equal(mirror[:n].cpu(), p[:n].cpu().to(torch.bfloat16))
    assert torch.allclose(ema[:n].cpu(), ema_ref, rtol=1e-6, atol=1e-7)
