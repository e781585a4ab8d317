"""The HBM-bound glue kernels of the detector trainer (csrc/yolo_train.hip, csrc/yolo_loss.hip, yv_sppf_pool of csrc/yolo_misc.hip),
each on its own at its edge shapes (yolo_glue_reference.py has the references, the bounds and the case lists;
test_yolo_glue_reference_cpu.py proves the gates on the CPU):
  A. yv_bn_stats / yv_bn_act_fwd / yv_bn_act_bwd: every element against an fp64 reference of the operands and a derived worst-case
     bound, gate 1.01, at C = 8 .. 1024 (256 to 2 row lanes), T around the unrolled-trip and rows-per-lane boundaries, 34 chunks
     and past the 2048-chunk cap, with and without activation, shortcut, batch statistics and running statistics; bit for bit on
     integer operands, and two calls give the same bits;
  B. yv_view_op (all seven modes), yv_maxpool5_bwd on the trainer's clipped P5 grids, yv_im2col3, yv_conv_weight_dgrad,
     yv_blob_nhwc8, yv_sppf_pool: bit for bit on small integers against plain-indexing references;
  C. yv_detect_loss: the box of every anchor (read from the workspace) and the set of positives exactly, every element of dbox,
     dcls and the four loss values within K EPS of its row's scale, K from a CPU measurement.
Outputs are pre-filled with a bf16-representable sentinel: what lies outside the live region (channels outside a view's slice, rows
past T, workspace past the size the *_ws_* function reports) must still hold it and every live element must have been written;
input rows past T and channels outside the slice are NaN and must not leak.  Each test prints its worst |got - ref| / B; the
module prints the worst per kernel at its end."""
import math

import pytest
import torch

import yolo_glue_reference as yg
from yolo_glue_reference import GATE, NAN_ROWS, SENTINEL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL_ROWS, TAIL_FLOATS, WS_BYTE = 3, 64, 0xA5
NAN = float("nan")
WORST = {}                                                           # kernel -> (ratio, case)


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    yield yvhip
    print("\nworst |got - ref| / bound per kernel over the case list (gate 1.01; yv_detect_loss: / (K EPS scale), gate 1):")
    for kernel, (r, case) in sorted(WORST.items()):
        print(f"  yolo-glue-bound {kernel} {r:.3f} at {case}")


def _note(kernel, r, case):
    print(f"{kernel} {case}: {r:.3f}")
    if r > WORST.get(kernel, (-1.0, None))[0]:
        WORST[kernel] = (r, case)


def _gate(kernel, case, got, ref, bound):
    r, i = yg.worst(got, ref, bound)
    _note(kernel, r, case)
    assert r <= GATE, f"{kernel} {case}: |got - ref| / bound = {r} at flat index {i}"


def _full(shape, fill=SENTINEL, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device=DEV)


def _vec(live, tail=TAIL_FLOATS):
    """device vector of live.numel() + tail sentinels; `live` (or an int: sentinels) in front"""
    n = live if isinstance(live, int) else live.numel()
    v = _full(n + tail)
    if not isinstance(live, int):
        v[:n] = live.reshape(-1).to(DEV)
    return v


def _untouched(t):
    return bool((t == SENTINEL).all())


def _written(t):
    return bool(torch.isfinite(t.float()).all()) and not bool((t == SENTINEL).any())


def _slice_buf(live, rows, Cn, ld, off, fill, extra):
    """(rows + extra, ld) bf16 on the device holding `fill`, and `live` (rows, Cn) (None: nothing) in columns [off, off + Cn)"""
    buf = _full((rows + extra, ld), fill, torch.bfloat16)
    if live is not None:
        buf[:rows, off:off + Cn] = live.reshape(rows, Cn).to(DEV).to(torch.bfloat16)
    return buf


def _outside_untouched(buf, rows, Cn, off):
    return _untouched(buf[rows:]) and _untouched(buf[:rows, :off]) and _untouched(buf[:rows, off + Cn:])


# ------------------------------------------------------------------------------------------------ A: BatchNorm + SiLU
def _geom(case):
    Cn = case[0]
    return (Cn, 0) if tuple(case[:3]) in yg.BN_BIG or case[1] > 100000 else (Cn + 16, 8)      # ld, channel offset


def _bn_stats(yv, z, ld, off, rm0=None, rv0=None):
    """-> dict of CPU tensors mean, rstd (run_mean, run_var); NaN around z, sentinels behind every output and the workspace"""
    T, Cn = z.shape
    zb = _slice_buf(z, T, Cn, ld, off, NAN, NAN_ROWS)
    mean, rstd = _vec(Cn), _vec(Cn)
    rm, rv = (None, None) if rm0 is None else (_vec(rm0), _vec(rv0))
    nws = yv.bn_ws_floats(T, Cn)
    assert nws == yg.bn_ws_floats(T, Cn)
    ws = _full(nws + TAIL_FLOATS)
    yv.bn_stats(yv.mview(zb, off, Cn), T, mean[:Cn], rstd[:Cn], None if rm is None else rm[:Cn], None if rv is None else rv[:Cn], ws[:nws])
    torch.cuda.synchronize()
    out = {"mean": mean, "rstd": rstd}
    if rm is not None:
        out.update(run_mean=rm, run_var=rv)
    assert _untouched(ws[nws:])
    for name, v in out.items():
        assert _untouched(v[Cn:]) and _written(v[:Cn]), name
    return {k: v[:Cn].cpu() for k, v in out.items()}


def _bn_fwd(yv, c, mean, rstd, ld, off, res, act):
    T, Cn = c["z"].shape
    zb = _slice_buf(c["z"], T, Cn, ld, off, NAN, NAN_ROWS)
    rb = _slice_buf(c["res"], T, Cn, ld, off, NAN, NAN_ROWS) if res else None
    ob = _slice_buf(None, T, Cn, ld, off, SENTINEL, TAIL_ROWS)
    yv.bn_act_fwd(yv.mview(zb, off, Cn), T, mean.to(DEV), rstd.to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV), yv.mview(ob, off, Cn),
                  res=yv.mview(rb, off, Cn) if res else None, act=act)
    torch.cuda.synchronize()
    assert _outside_untouched(ob, T, Cn, off) and _written(ob[:T, off:off + Cn])
    return ob[:T, off:off + Cn].cpu()


def _bn_bwd(yv, c, mean, rstd, ld, off, act, bs):
    """-> dz (T, C) bf16, dgamma, dbeta (C) on the CPU"""
    T, Cn = c["z"].shape
    zb = _slice_buf(c["z"], T, Cn, ld, off, NAN, NAN_ROWS)
    db = _slice_buf(c["da"], T, Cn, ld, off, NAN, NAN_ROWS)
    ob = _slice_buf(None, T, Cn, ld, off, SENTINEL, TAIL_ROWS)
    dga, dbe = _vec(Cn), _vec(Cn)
    nws = yv.bn_ws_floats(T, Cn)
    ws = _full(nws + TAIL_FLOATS)
    yv.bn_act_bwd(yv.mview(db, off, Cn), yv.mview(zb, off, Cn), T, mean.to(DEV), rstd.to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV),
                  dga[:Cn], dbe[:Cn], yv.mview(ob, off, Cn), ws[:nws], act=act, batch_stats=bool(bs))
    torch.cuda.synchronize()
    assert _untouched(ws[nws:]) and _untouched(dga[Cn:]) and _untouched(dbe[Cn:]) and _written(dga[:Cn]) and _written(dbe[:Cn])
    assert _outside_untouched(ob, T, Cn, off) and _written(ob[:T, off:off + Cn])
    return ob[:T, off:off + Cn].cpu(), dga[:Cn].cpu(), dbe[:Cn].cpu()


@pytest.mark.parametrize("case", yg.BN_CASES, ids=str)
def test_bn_stats(yv, case):
    """with and without running statistics (T = 1 with them: the unbiased-variance rule has no T - 1 to divide by)"""
    c = yg.bn_case(*case)
    ld, off = _geom(case)
    ref = yg.bn_stats_reference(c["z"], c["rm0"], c["rv0"])
    got = _bn_stats(yv, c["z"], ld, off, c["rm0"], c["rv0"])
    for name in ("mean", "rstd", "run_mean", "run_var"):
        _gate("bn_stats " + name, case, got[name], ref[name], ref["b_" + name])
    again = _bn_stats(yv, c["z"], ld, off, c["rm0"], c["rv0"])
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)       # bitwise reproducible
    if case not in yg.BN_BIG:
        plain = _bn_stats(yv, c["z"], ld, off)
        assert torch.equal(plain["mean"], got["mean"]) and torch.equal(plain["rstd"], got["rstd"])
    if case[2] == "values":
        assert float(got["rstd"][0]) == float(torch.tensor(1.0 / math.sqrt(yg.f32v(yg.BN_EPS)), dtype=torch.float64).float())       # var = 0
        for name, ch in (("ratio8", 1), ("ratio64", 2)):
            ratio, acc = yg.bn_stats_accuracy(c["z"], ch)
            err = abs(float(got["rstd"][ch]) - float(ref["rstd"][ch])) / float(ref["rstd"][ch])
            print(f"bn_stats accuracy {case} |mean| / std = {ratio:.1f}: B_rstd / rstd = {acc:.3e}, kernel |rstd - ref| / rstd = {err:.3e}")


@pytest.mark.parametrize("case", yg.BN_CASES, ids=str)
def test_bn_act_fwd(yv, case):
    c = yg.bn_case(*case)
    ld, off = _geom(case)
    mean, rstd = yg.bn_operand_stats(c["z"])
    for act, res in ([(1, True)] if case in yg.BN_BIG else yg.BN_OPTS):
        got = _bn_fwd(yv, c, mean, rstd, ld, off, res, act)
        _gate("bn_act_fwd", (*case, f"act={act} res={int(res)}"), got.float(),
              *yg.bn_act_fwd_reference(c["z"], mean, rstd, c["gamma"], c["beta"], c["res"] if res else None, act))
    assert torch.equal(got.view(torch.int16), _bn_fwd(yv, c, mean, rstd, ld, off, res, act).view(torch.int16))


@pytest.mark.parametrize("case", yg.BN_CASES, ids=str)
def test_bn_act_bwd(yv, case):
    c = yg.bn_case(*case)
    ld, off = _geom(case)
    mean, rstd = yg.bn_operand_stats(c["z"])
    for act, bs in ([(1, 1)] if case in yg.BN_BIG else yg.BN_BWD_OPTS):
        dz, dga, dbe = _bn_bwd(yv, c, mean, rstd, ld, off, act, bs)
        ref = yg.bn_act_bwd_reference(c["da"], c["z"], mean, rstd, c["gamma"], c["beta"], act, bs)
        tag = (*case, f"act={act} bs={bs}")
        _gate("bn_act_bwd dz", tag, dz.float(), ref["dz"], ref["b_dz"])
        _gate("bn_act_bwd dgamma", tag, dga, ref["dgamma"], ref["b_dgamma"])
        _gate("bn_act_bwd dbeta", tag, dbe, ref["dbeta"], ref["b_dbeta"])
    dz2, dga2, dbe2 = _bn_bwd(yv, c, mean, rstd, ld, off, act, bs)
    assert torch.equal(dz.view(torch.int16), dz2.view(torch.int16)) and torch.equal(dga.view(torch.int32), dga2.view(torch.int32))
    assert torch.equal(dbe.view(torch.int32), dbe2.view(torch.int32))


@pytest.mark.parametrize("Cn,T", [(8, 257), (24, 86), (1024, 33), (16, 8449), (8, 524289), (8, 1)])
def test_bn_exact_on_integers(yv, Cn, T):
    """integer z: mean == f32(sum / T), rstd and the running estimates are the finaliser's formulas in double, rounded once;
    dbeta of integer da with act 0; dz == bf16(gamma rstd da) with frozen statistics, act 0 and gamma rstd = 2"""
    c = yg.bn_case(Cn, T, "rand", exact=True)
    ld, off = _geom((Cn, T))
    got = _bn_stats(yv, c["z"], ld, off, c["rm0"], c["rv0"])
    mean, rstd, rm, rv = yg.bn_stats_exact(c["z"], c["rm0"], c["rv0"])
    assert torch.equal(got["mean"], mean) and torch.equal(got["mean"], (c["z"].double().sum(0) / T).float())
    assert torch.equal(got["rstd"], rstd) and torch.equal(got["run_mean"], rm) and torch.equal(got["run_var"], rv)
    one = torch.ones(Cn)
    for bs in (0, 1):
        dz, _, dbe = _bn_bwd(yv, c, one, one, ld, off, 0, bs)
        assert torch.equal(dbe, c["da"].sum(0)), bs
    dz, _, _ = _bn_bwd(yv, c, one, one, ld, off, 0, 0)
    assert torch.equal(dz, yg.bf(2.0 * c["da"]))


def test_bn_act_fwd_rounds_twice_exactly(yv):
    """v = z + 2^-9 and res on a lattice of 2^-9: bf16(bf16(v) + res), not bf16(v + res)"""
    g = torch.Generator().manual_seed(1)
    z = yg.int_tensor((86, 24), g, 1, 1)
    res = torch.randint(0, 8, (86, 24), generator=g).float() * 2.0 ** -9
    c = {"z": z, "res": res, "gamma": torch.ones(24), "beta": torch.full((24,), 2.0 ** -9)}
    got = _bn_fwd(yv, c, torch.zeros(24), torch.ones(24), 40, 8, True, 0)
    assert torch.equal(got, yg.bf(yg.bf(z + c["beta"]).float() + res))
    assert not torch.equal(got, yg.bf(z + c["beta"] + res))


# ------------------------------------------------------------------------------------------------ B: exact kernels
@pytest.mark.parametrize("Cn", [8, 24])
@pytest.mark.parametrize("B,H,W", yg.VIEW_SHAPES)
def test_view_op_exact(yv, B, H, W, Cn):
    """all seven modes, source and destination both slices of wider buffers; mode 3 accumulates into a non-zero destination, the
    ring of mode 6 and the zeros of modes 4 and 5 overwrite the sentinel"""
    for mode in range(7):
        c = yg.view_case(mode, B, H, W, Cn)
        (SH, SW), (DH, DW) = yg.view_src_dims(mode, H, W), yg.view_dst_dims(mode, H, W)
        ns, nd = B * SH * SW, B * DH * DW
        sb = _slice_buf(c["src"], ns, Cn, Cn + 16, 8, NAN, NAN_ROWS)
        db = _slice_buf(c["dst0"] if mode in (1, 3) else None, nd, Cn, Cn + 24, 16, SENTINEL, TAIL_ROWS)
        yv.view_op(mode, None if mode == 5 else yv.mview(sb, 8, Cn), yv.mview(db, 16, Cn), B, H, W)
        torch.cuda.synchronize()
        ref = yg.view_op_reference(mode, c["src"], c["dst0"], H, W)
        assert _outside_untouched(db, nd, Cn, 16), mode
        assert torch.equal(db[:nd, 16:16 + Cn].float().cpu().view(B, DH, DW, Cn), ref), mode


@pytest.mark.parametrize("Cn", [8, 24])
@pytest.mark.parametrize("H,W", yg.POOL_SHAPES)
def test_maxpool5_bwd_exact(yv, H, W, Cn):
    """1 x 1 to 7 x 4: every window is clipped.  dout and din are two channel slices of one buffer, din is non-zero on entry, the
    workspace is exactly B H W C bytes with a guard behind it"""
    B = 2
    n = B * H * W
    for pattern in yg.POOL_PATTERNS:
        c = yg.pool_case(H, W, Cn, pattern)
        xb = _slice_buf(c["x"], n, Cn, Cn + 16, 8, NAN, NAN_ROWS)
        gb = _slice_buf(c["dout"], n, Cn, 2 * Cn + 16, 0, SENTINEL, TAIL_ROWS)
        gb[:n, Cn + 8:2 * Cn + 8] = c["din0"].reshape(n, Cn).to(DEV).to(torch.bfloat16)
        ws = torch.full((n * Cn + 64,), WS_BYTE, dtype=torch.uint8, device=DEV)
        x, dout, din = yv.mview(xb, 8, Cn), yv.mview(gb, 0, Cn), yv.mview(gb, Cn + 8, Cn)
        yv.check(yv.lib.yv_maxpool5_bwd(x.ptr, x.ld, dout.ptr, dout.ld, din.ptr, din.ld, B, H, W, Cn, yv._p(ws), n * Cn, yv._st()),
                 "yv_maxpool5_bwd")
        torch.cuda.synchronize()
        ref = yg.maxpool5_bwd_reference(c["x"], c["dout"], c["din0"])
        assert bool((ws[n * Cn:] == WS_BYTE).all()) and _untouched(gb[n:]) and _untouched(gb[:n, Cn:Cn + 8]) and _untouched(gb[:n, 2 * Cn + 8:])
        assert torch.equal(gb[:n, :Cn].float().cpu(), c["dout"].reshape(n, Cn))
        assert torch.equal(gb[:n, Cn + 8:2 * Cn + 8].float().cpu().view(B, H, W, Cn), ref), pattern


@pytest.mark.parametrize("Cn", [8, 24])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Hin,Win", yg.IM2COL_SHAPES)
def test_im2col3_exact(yv, Hin, Win, stride, Cn):
    B = 2
    x = yg.int_tensor((B, Hin, Win, Cn), torch.Generator().manual_seed(Hin * 9 + Win + Cn))
    ref = yg.im2col3_reference(x, stride)
    T = ref.shape[0]
    xb = _slice_buf(x, B * Hin * Win, Cn, Cn + 16, 8, NAN, NAN_ROWS)
    col = _full((T + TAIL_ROWS, 9 * Cn), SENTINEL, torch.bfloat16)
    yv.im2col3(yv.mview(xb, 8, Cn), B, Hin, Win, stride, col)
    torch.cuda.synchronize()
    assert _untouched(col[T:]) and torch.equal(col[:T].float().cpu(), ref)


@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("Cout,Cin", yg.WDGRAD_SHAPES)
def test_conv_weight_dgrad_exact(yv, Cout, Cin, taps):
    w = yg.int_tensor((Cout, taps, Cin), torch.Generator().manual_seed(Cout + Cin + taps))
    n = Cout * taps * Cin
    wd = _full(n + TAIL_FLOATS, SENTINEL, torch.bfloat16)
    yv.conv_weight_dgrad(w.to(torch.bfloat16).to(DEV), Cout, taps, Cin, wd)
    torch.cuda.synchronize()
    assert _untouched(wd[n:]) and torch.equal(wd[:n].float().cpu().view(Cin, taps, Cout), yg.weight_dgrad_reference(w))


@pytest.mark.parametrize("pixels", yg.BLOB_PIXELS)
def test_blob_nhwc8_exact(yv, pixels):
    img = yg.blob_case(pixels)
    out = _full((pixels + TAIL_ROWS, 8), SENTINEL, torch.bfloat16)
    yv.blob_nhwc8(img.to(DEV), out)
    torch.cuda.synchronize()
    assert _untouched(out[pixels:]) and torch.equal(out[:pixels].cpu().view(torch.int16), yg.blob_reference(img).view(torch.int16))


@pytest.mark.parametrize("c", [8, 24])
@pytest.mark.parametrize("H,W", yg.SPPF_SHAPES)
def test_sppf_pool_exact(yv, H, W, c):
    B, ld = 2, 4 * c + 8
    n = B * H * W
    x = yg.int_tensor((B, H, W, c), torch.Generator().manual_seed(H + W + c), -100, 100)
    buf = _slice_buf(x, n, c, ld, 0, SENTINEL, TAIL_ROWS)
    yv.check(yv.lib.yv_sppf_pool(yv._p(buf), B, H, W, ld, c, yv._st()), "yv_sppf_pool")
    torch.cuda.synchronize()
    assert _untouched(buf[n:]) and _untouched(buf[:n, 4 * c:])
    assert torch.equal(buf[:n, :4 * c].float().cpu().view(B, H, W, 4 * c), yg.sppf_reference(x))


# ------------------------------------------------------------------------------------------------ C: detection loss
def _detect_loss(yv, c):
    """-> dict of CPU tensors: loss (4), dbox, dcls (lists), tgt (B, A) from the workspace.  Boxes and labels past an image's count
    are NaN / 9999 on the device: they must not be read"""
    B, G, A, S, nc, ncp = c["B"], c["G"], c["A"], c["S"], c["nc"], c["ncp"]
    live = torch.arange(G)[None] < c["cnt"][:, None]
    gtb = torch.where(live[..., None], c["gtb"], torch.full_like(c["gtb"], NAN)).to(DEV)
    gtl = torch.where(live, c["gtl"], torch.full_like(c["gtl"], 9999)).to(DEV)
    box, cls = [t.to(DEV) for t in c["box"]], [t.to(DEV) for t in c["cls"]]
    dbox = [_full((t.shape[0] + TAIL_ROWS, 64)) for t in box]
    dcls = [_full((t.shape[0] + TAIL_ROWS, ncp)) for t in cls]
    loss = _vec(4)
    nws = yv.detect_loss_ws_bytes(B, A, G)
    assert nws == yg.loss_ws_bytes(B, A, G)
    ws = torch.full((nws + 256,), WS_BYTE, dtype=torch.uint8, device=DEV)
    yv.detect_loss(box, cls, dbox, dcls, B, S, nc, ncp, gtb, gtl, c["cnt"].to(DEV), loss[:4], ws[:nws])
    torch.cuda.synchronize()
    assert bool((ws[nws:] == WS_BYTE).all()) and _untouched(loss[4:]) and _written(loss[:4])
    for got, src in zip(dbox + dcls, box + cls):
        assert _untouched(got[src.shape[0]:]) and _written(got[:src.shape[0]])                 # every row of dbox and dcls is written
    o, n = yg.loss_ws_layout(B, A, G)["tgt"]
    tgt = ws[:nws].cpu().view(torch.int32)[o:o + n].view(B, A).long()
    return {"loss": loss[:4].cpu(), "dbox": [d[:t.shape[0]].cpu() for d, t in zip(dbox, box)],
            "dcls": [d[:t.shape[0]].cpu() for d, t in zip(dcls, cls)], "tgt": tgt}


@pytest.mark.parametrize("name", list(yg.LOSS_CASES))
def test_detect_loss(yv, name):
    c = yg.loss_case(name)                                            # asserts every margin
    ref = c["ref"]
    got = _detect_loss(yv, c)
    assert torch.equal(got["tgt"], ref["tgt"]), "an anchor is assigned to another box than in the reference"
    rows = torch.cat([(d != 0).any(1).view(c["B"], -1) for d in got["dbox"]], 1)
    assert torch.equal(rows, (ref["tgt"] >= 0) & (ref["weight"] > 0))                         # the positives, exactly
    for d in got["dcls"]:
        assert bool((d[:, c["nc"]:] == 0).all())
    again = _detect_loss(yv, c)
    for k in ("dbox", "dcls"):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[k], again[k])), k
    assert torch.equal(got["loss"].view(torch.int32), again["loss"].view(torch.int32))
    for out, r in yg.loss_ratios(got, ref).items():
        _note("detect_loss " + out, r / yg.loss_k(out), name)
        assert r <= yg.loss_k(out), f"{name} {out}: |got - ref| / (EPS scale) = {r}, K = {yg.loss_k(out)}"
