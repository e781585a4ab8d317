"""yv_conv2d_bnbwd + yv_bn_act_bwd_finish (YoloTrainer(fused_bn_bwd=True)): the data gradient of yv_conv2d_ws that also writes, per
tile, the two sums of the BatchNorm backward of the block whose output gradient it stores - on every kernel instance a
single-source convolution can take and in both epilogue forms.

EXACT cases use the conventions of test_gpu_conv_stats.py (operands from {-1, 0, 1}, thinned weights, a sentinel around every
output, the route asserted before it runs) plus a residual from [-4, 4] and a producer pre-activation z from [-3, 3] with act = 0,
mean = 0, rstd = 1, gamma = 1, beta = 0: then xhat = z, g = da, both exact small integers, and every column sum of |da| and of
|da * z| stays below 2^24 (computed in int64 and asserted before anything is launched), so every f32 partial sum, in any order, is
an exact integer and the comparisons are equalities.

RANDOM cases (act = 1) are gated against yolo_glue_reference.bn_act_bwd_reference in fp64 on the STORED da, with that module's
GATE = 1.01 times its derived bound, its two-stage summation depth replaced by the fused path's own (fused_sum_rel):

  d1, the f32 additions a term passes through in the epilogue (gemm.hip).  A 128-row tile is WM row groups of MF * 16 rows
  (MF = 8 / WM; WM = 4 on the 16-, 32- and 64-wide tiles, 2 on the 128-wide ones).
    staged epilogue (epilogue_staged): a lane stores rows (lane >> 3) + 8 * it, it < MF * 2, and adds each to cs / cq in that order:
      MF * 2 additions; finish_tile's xor butterfly over d = 8, 16, 32: 3 additions; the WM waves in wave order: WM additions.
      d1 = 2 MF + 3 + WM  (11 at WM = 4, 13 at WM = 2)
    direct epilogue (epilogue, one 16-column fragment at a time): a lane stores rows j * 16 + fr, j < MF: MF additions; the
      butterfly over d = 1, 2, 4, 8: 4 additions; the WM waves: WM additions.
      d1 = MF + 4 + WM    (10 at either WM)
    Above 2048 tiles bn_stats_fold_kernel writes its double sum of a group of tiles back as ONE float: d1 + 1.
  The bound uses the larger of the two forms for the tile width, so it does not depend on which epilogue ran.
  d2, the double additions behind it: the fold's group = ceil(tiles / 2048) (0 without a fold), then chunk_sums of
  bn_bwd_final_kernel, ceil(chunks / 32) + 32 (yolo_train.hip; chunks = tiles, or the fold's chunk count).
Nothing is fitted to the kernel's output; two runs must give the same bits."""
import math

import pytest
import torch

import yolo_glue_reference as ref
from test_gpu_conv_routes import DEV, SENTINEL, Options, bf
from test_gpu_conv_stats import make_int_data, tile_sums, tiles_of

pytestmark = pytest.mark.gpu
PAD = 192                       # floats allocated behind yv_conv_bnbwd_ws_floats: must keep the sentinel
NAN_ROWS = 3                    # rows of NaN behind T in z: they must add nothing


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def bcase(name, B, H, W, k, cin, cout, kernel, staged, out=(0, None), res=(0, None), z=(0, None), src=(0, None), inplace=False, **opts):
    """out / res / z / src: (channel offset, pixel stride or None = dense).  kernel, staged: the route that must run.  inplace: the
    residual IS the output view, as the trainer accumulates.  opts: library options of the case."""
    return dict(name=name, B=B, H=H, W=W, k=k, s=1, srcs=[(cin, 0, src[0], src[1] or cin)], cout=cout, kernel=kernel, staged=staged,
                out=(out[0], out[1] or cout), res=(res[0], res[1] or cout), z=(z[0], z[1] or cout), inplace=inplace, opts=opts)


def bcases(yv):
    """All nine instances; the 64- and 128-wide igemm tiles in both epilogue forms (direct under "staged_epilogue" = 0)."""
    I16, I32, I64, I128 = yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_128
    D642, D643, D644, D1282, D1283 = yv.CONV_DMA_64_2, yv.CONV_DMA_64_3, yv.CONV_DMA_64_4, yv.CONV_DMA_128_2, yv.CONV_DMA_128_3
    return [
        bcase("igemm16_T240", 2, 10, 12, 3, 32, 16, I16, False),
        bcase("igemm32_slices", 1, 7, 5, 3, 24, 24, I32, False, out=(8, 40), res=(16, 48), z=(8, 56), src=(8, 40)),
        bcase("igemm64_staged", 2, 11, 9, 3, 48, 64, I64, True),
        bcase("igemm64_direct", 2, 11, 9, 3, 48, 64, I64, False, staged_epilogue=0),
        bcase("igemm128_staged_ragged_n", 2, 17, 9, 3, 32, 96, I128, True, inplace=True),
        bcase("igemm128_direct_n144", 1, 13, 13, 1, 96, 144, I128, False, staged_epilogue=0),
        bcase("dma64_1x1_n80_T270", 2, 9, 15, 1, 128, 80, D643, True),
        bcase("dma64_T5_one_ragged_tile", 5, 1, 1, 3, 64, 64, D643, True),
        bcase("dma64_T1122_slices_inplace", 2, 33, 17, 3, 192, 144, D643, True, out=(16, 176), res=(16, 176), z=(8, 160), inplace=True),
        bcase("dma128_320x320_n80", 1, 320, 320, 1, 64, 80, D1282, True),
        bcase("fold_T266240_2080_tiles_c16", 1, 512, 520, 1, 16, 16, I16, False),
        bcase("dma64_two_stage", 2, 20, 20, 3, 64, 64, D642, True, conv_dma=1),
        bcase("dma128_three_stage", 2, 20, 20, 3, 128, 128, D1283, True, conv_dma=3),
        bcase("dma64_four_stage", 2, 20, 20, 3, 128, 128, D644, True, conv_dma=4),
    ]


def case_names():
    import yvhip
    return [c["name"] for c in bcases(yvhip)]


def find(yv, name):
    return next(c for c in bcases(yv) if c["name"] == name)


def r64(n):
    return (n + 63) // 64 * 64


def route_of(yv, c, flags):
    (cin, _, _, in_ld), = c["srcs"]
    return yv.conv_bnbwd_route(c["B"], c["H"], c["W"], c["k"], 1, cin, c["cout"], in_ld=in_ld, out_ld=c["out"][1], res_ld=c["res"][1],
                               ldz=c["z"][1], flags=flags)


def add_bn_operands(c, d, seed, exact):
    """The residual, the producer's z (with NaN rows behind T) and its constants; exact: the integer setting of the module docstring."""
    g = torch.Generator().manual_seed(seed)
    T, C = c["B"] * c["H"] * c["W"], c["cout"]
    rows = r64(T) + NAN_ROWS
    if exact:
        d["res"] = torch.randint(-4, 5, (T, c["res"][1]), generator=g).float()
        z = torch.randint(-3, 4, (rows, c["z"][1]), generator=g).float()
        d["consts"] = [torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)]
    else:
        d["res"] = bf(torch.randn(T, c["res"][1], generator=g)).float()
        z = bf(torch.randn(rows, c["z"][1], generator=g) * 1.5 + 0.3).float()
        mean, rstd = ref.bn_operand_stats(z[:T, c["z"][0]:c["z"][0] + C])
        d["consts"] = [mean, rstd, 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)]
    z[T:] = float("nan")
    d["pz"] = z
    return d


def to_dev(d):
    d["x_d"], d["w_d"], d["bias_d"] = bf(d["x"]).to(DEV), bf(d["w"]).to(DEV), d["bias"].to(DEV)
    d["res_d"], d["pz_d"], d["consts_d"] = bf(d["res"]).to(DEV), bf(d["pz"]).to(DEV), [t.float().to(DEV) for t in d["consts"]]
    return d


def out_buffer(c, d):
    """The output buffer before the call: the sentinel; in place, the residual's values in the output's channels."""
    T, (off, ld) = c["B"] * c["H"] * c["W"], c["out"]
    out = torch.full((T, ld), SENTINEL, dtype=torch.bfloat16, device=DEV)
    if c["inplace"]:
        out[:, off:off + c["cout"]] = d["res_d"][:, c["res"][0]:c["res"][0] + c["cout"]]
    return out


def run_pair(yv, c, d, act, fused, ws_floats=None):
    """conv_view_bnbwd (fused) or conv_view of the case; returns (out buffer, stats_ws or None, need)."""
    T, C = c["B"] * c["H"] * c["W"], c["cout"]
    (cin, up, soff, _), = c["srcs"]
    out = out_buffer(c, d)
    ov = yv.mview(out, c["out"][0], C)
    rv = ov if c["inplace"] else yv.mview(d["res_d"], c["res"][0], C)
    args = (yv.view(d["x_d"], soff, cin, up), c["B"], c["H"], c["W"], c["k"], 1, d["w_d"], C, ov)
    if not fused:
        yv.conv_view(*args, res=rv, bias=d["bias_d"])
        torch.cuda.synchronize()
        return out, None, 0
    need = yv.conv_bnbwd_ws_floats(T, C)
    ws = torch.full((need + PAD if ws_floats is None else ws_floats,), SENTINEL, device=DEV)
    yv.conv_view_bnbwd(*args, yv.mview(d["pz_d"], c["z"][0], C), *d["consts_d"], ws, act=act, res=rv, bias=d["bias_d"])
    torch.cuda.synchronize()
    return out, ws, need


def bwd_outputs(yv, c, d, da, T, act, ws=None):
    """dgamma, dbeta, dz of bn_act_bwd_finish on the partials `ws`, or (ws None) of bn_act_bwd, from the stored gradient da."""
    C = c["cout"]
    dg, db = torch.full((C,), SENTINEL, device=DEV), torch.full((C,), SENTINEL, device=DEV)
    dz = torch.full((r64(T), C + 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    zv, dzv = yv.mview(d["pz_d"], c["z"][0], C), yv.mview(dz, 8, C)
    if ws is None:
        yv.bn_act_bwd(da, zv, T, *d["consts_d"], dg, db, dzv, torch.zeros(yv.bn_ws_floats(T, C), device=DEV), act=act)
    else:
        yv.bn_act_bwd_finish(da, zv, T, *d["consts_d"], dg, db, dzv, ws, act=act)
    torch.cuda.synchronize()
    assert bool((dz[:, :8] == SENTINEL).all()) and bool((dz[T:] == SENTINEL).all()), "dz written outside its rows / channels"
    return dg, db, dz[:T, 8:]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", case_names())
def test_bnbwd_exact_integer(yv, name):
    """Every instance and epilogue form: `out` is the exact integer reference and what conv_view writes, bit for bit; the channels
    outside the slice and the floats behind yv_conv_bnbwd_ws_floats keep the sentinel; every tile partial equals the int64 sum over
    that tile's rows (the NaN rows of z behind T add nothing); dgamma, dbeta and dz of bn_act_bwd_finish equal yv_bn_act_bwd's on
    the stored da bit for bit."""
    c = find(yv, name)
    seed = sum(map(ord, name))
    d = add_bn_operands(c, make_int_data(c, seed), seed + 1, exact=True)
    T, C, off = c["B"] * c["H"] * c["W"], c["cout"], c["out"][0]
    da = d["z"] + d["res"][:, c["res"][0]:c["res"][0] + C].to(torch.int64)            # conv + bias + residual, int64
    pz = d["pz"][:T, c["z"][0]:c["z"][0] + C].to(torch.int64)
    assert int(da.abs().max()) <= 256                                                 # exact in bf16, whichever rounding order
    ratio = max(int(da.abs().sum(0).max()), int((da * pz).abs().sum(0).max())) / 2 ** 24
    assert ratio < 1.0, ratio
    print(f"\n{name}: T = {T}, {tiles_of(T)} tiles, max column sum of |da|, |da z| / 2^24 = {ratio:.3f}")
    to_dev(d)
    flags = yv.EPI_BIAS | yv.EPI_RES_BF16
    with Options(yv, **c["opts"]):
        r = route_of(yv, c, flags)
        # (`use` is the trainer's business: the 320 x 320 case is one the route sends back on time; the call itself must be right)
        assert (r.kernel, r.staged, r.tiles, r.splitk) == (c["kernel"], c["staged"], tiles_of(T), False), (name, r)
        assert r.use == (T < 100000 or r.kernel < yv.CONV_IGEMM_32), (name, r)
        out, ws, need = run_pair(yv, c, d, 0, fused=True)
        plain, _, _ = run_pair(yv, c, d, 0, fused=False)
    got = out[:, off:off + C]
    assert torch.equal(got.cpu(), bf(da.float())), "out differs from the integer reference"
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), "out differs from conv_view's"
    outside = torch.cat([out[:, :off], out[:, off + C:]], -1)
    assert bool((outside == SENTINEL).all()), "wrote outside its channels"
    n = tiles_of(T)
    assert need == yv.conv_stats_ws_floats(T, C) + 2 * C and need >= n * 2 * C
    assert bool((ws[n * 2 * C:] == SENTINEL).all()), "the convolution wrote behind its tile partials"
    part = ws[:n * 2 * C].view(n, 2, C).cpu().double()
    assert torch.equal(part[:, 0], tile_sums(da).double()), "a tile's sum of g"
    assert torch.equal(part[:, 1], tile_sums(da * pz).double()), "a tile's sum of g * xhat"
    dav = yv.mview(out, off, C)
    dg, db, dz = bwd_outputs(yv, c, d, dav, T, 0, ws)
    assert bool((ws[need:] == SENTINEL).all()), "bn_act_bwd_finish wrote behind yv_conv_bnbwd_ws_floats"
    dg2, db2, dz2 = bwd_outputs(yv, c, d, dav, T, 0)
    assert torch.equal(db.cpu().double(), da.sum(0).double()) and torch.equal(dg.cpu().double(), (da * pz).sum(0).double())
    assert torch.equal(dg, dg2) and torch.equal(db, db2), "dgamma / dbeta differ from yv_bn_act_bwd's"
    assert torch.equal(dz.view(torch.int16), dz2.view(torch.int16)), "dz differs from yv_bn_act_bwd's"


# ------------------------------------------------------------------------------------------------ 2
def fused_sum_rel(T, width):
    """d1 EPS + d2 EPS64 of the module docstring for T rows on tiles `width` columns wide."""
    wm = 2 if width == 128 else 4
    mf = 8 // wm
    tiles = tiles_of(T)
    group = (tiles + 2047) // 2048
    chunks = (tiles + group - 1) // group
    d1 = max(2 * mf + 3 + wm, mf + 4 + wm) + (1 if tiles > 2048 else 0)
    d2 = (group if tiles > 2048 else 0) + (chunks + 31) // 32 + 32
    return d1 * ref.EPS + d2 * ref.EPS64


def width_of(yv, kernel):
    return {yv.CONV_IGEMM_16: 16, yv.CONV_IGEMM_32: 32, yv.CONV_IGEMM_128: 128, yv.CONV_DMA_128_2: 128, yv.CONV_DMA_128_3: 128}.get(kernel, 64)


def fused_reference(monkeypatch, da, z, consts, width, act=1):
    """bn_act_bwd_reference with the fused path's summation depth in place of chan_reduce_kernel's."""
    monkeypatch.setattr(ref, "_sum_rel", lambda T, C: fused_sum_rel(T, width))
    return ref.bn_act_bwd_reference(da, z, *consts, act=act, batch_stats=1)


def gate(got, r, what):
    err, bound = (got.double() - r[what]).abs(), ref.GATE * r["b_" + what]
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {what}: worst error / gate = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("name", ["igemm32_slices", "igemm64_direct", "igemm128_staged_ragged_n", "dma64_T1122_slices_inplace"])
def test_bnbwd_random_data_silu(yv, name, monkeypatch):
    """randn operands, randn / sqrt(K) weights, a randn residual, act = 1, batch statistics of z as mean / rstd.  dgamma, dbeta and
    every element of dz within GATE times the derived bound of the fp64 reference on the stored da; two runs give the same bits;
    `out` is conv_view's."""
    c = find(yv, name)
    g = torch.Generator().manual_seed(len(name))
    (cin, _, _, ld), = c["srcs"]
    K = c["k"] ** 2 * cin
    T, C, off = c["B"] * c["H"] * c["W"], c["cout"], c["out"][0]
    d = dict(x=torch.randn(c["B"], c["H"], c["W"], ld, generator=g), w=torch.randn(C, K, generator=g) / math.sqrt(K),
             bias=torch.randn(C, generator=g))
    to_dev(add_bn_operands(c, d, len(name) + 1, exact=False))
    runs = []
    with Options(yv, **c["opts"]):
        r = route_of(yv, c, yv.EPI_BIAS | yv.EPI_RES_BF16)
        assert (r.kernel, r.staged) == (c["kernel"], c["staged"]), (name, r)
        for _ in range(2):
            out, ws, need = run_pair(yv, c, d, 1, fused=True)
            runs.append((out, ws[:tiles_of(T) * 2 * C].clone(), bwd_outputs(yv, c, d, yv.mview(out, off, C), T, 1, ws)))
        plain, _, _ = run_pair(yv, c, d, 1, fused=False)
    (out, part, res), (out_b, part_b, res_b) = runs
    assert torch.equal(out.view(torch.int16), out_b.view(torch.int16)) and torch.equal(part, part_b)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16)) for a, b in zip(res, res_b))
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), "out differs from conv_view's"
    assert not bool(torch.isnan(part).any()), "NaN rows of z behind T were added"
    da = out[:, off:off + C].cpu()
    z = d["pz"][:T, c["z"][0]:c["z"][0] + C]
    want = fused_reference(monkeypatch, da, bf(z), d["consts"], width_of(yv, c["kernel"]))
    print(f"\n{name}: T = {T}, C = {C}")
    dg, db, dz = (t.cpu() for t in res)
    gate(dg, want, "dgamma"); gate(db, want, "dbeta"); gate(dz, want, "dz")


# ------------------------------------------------------------------------------------------------ 3
def test_bnbwd_rejects(yv):
    """The argument checks of tests/test_bn_bwd_fused_cpu.py with real tensors: a forbidden flag, a short workspace and a z stride
    that does not cover the channels raise and leave `out` and `stats_ws` untouched."""
    c = find(yv, "dma64_1x1_n80_T270")
    d = to_dev(add_bn_operands(c, make_int_data(c, seed=3), 4, exact=True))
    T, C = c["B"] * c["H"] * c["W"], c["cout"]
    need = yv.conv_bnbwd_ws_floats(T, C)
    out = torch.full((T, C), SENTINEL, dtype=torch.bfloat16, device=DEV)
    (cin, up, soff, _), = c["srcs"]

    def call(ws, flags=0, zc=C):
        zv = yv.mview(d["pz_d"], 0, C)
        zv.ld = zc if zc != C else zv.ld
        yv.conv_view_bnbwd(yv.view(d["x_d"], soff, cin, up), c["B"], c["H"], c["W"], c["k"], 1, d["w_d"], C, yv.mview(out), zv,
                           *d["consts_d"], ws, act=0, bias=d["bias_d"], flags=flags)

    with Options(yv):
        for flags, floats, zc in ((yv.EPI_SILU, need, C), (yv.EPI_OUT_F32, need, C), (yv.EPI_GELU, need, C), (0, need - 1, C),
                                  (0, yv.conv_stats_ws_floats(T, C), C), (0, need, C - 8), (0, need, C + 4)):
            ws = torch.full((floats,), SENTINEL, device=DEV)
            with pytest.raises(yv.YvError):
                call(ws, flags, zc)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all()), (flags, floats, zc)
        with pytest.raises(yv.YvError):                                  # the finaliser: a workspace below the size function
            yv.bn_act_bwd_finish(yv.mview(out), yv.mview(d["pz_d"], 0, C), T, *d["consts_d"], torch.zeros(C, device=DEV),
                                 torch.zeros(C, device=DEV), yv.mview(torch.zeros_like(out)), torch.zeros(need - 1, device=DEV), act=0)
        ws = torch.full((need,), SENTINEL, device=DEV)                  # the same call with nothing wrong runs
        call(ws)
        torch.cuda.synchronize()
        assert not bool((out == SENTINEL).any()) and not bool((ws[:need - 2 * C] == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ 4
SCALE, NC, SIZE, BATCH = "n", 5, 64, 2
PAIR = ("model.2.m.0.cv2", "model.2.m.0.cv1")                            # (consumer, producer)


def trainer_pair(yv, **kw):
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    sd = init_yolo_train_state(SCALE, NC, seed=3)
    return YoloTrainer({k: v.clone() for k, v in sd.items()}, scale=SCALE, nc=NC, size=SIZE, batch=BATCH, **kw)


def run_step(tr, seed=11):
    """forward, the loss of two boxes per image, backward; no optimiser step."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), generator=g, dtype=torch.uint8).to(DEV)
    ctr, wh = torch.rand(BATCH, 2, 2, generator=g) * (SIZE - 30) + 15, torch.rand(BATCH, 2, 2, generator=g) * 20 + 8
    tr.forward(img)
    tr.loss(torch.cat([ctr - wh / 2, ctr + wh / 2], -1).to(DEV), torch.randint(0, NC, (BATCH, 2), generator=g, dtype=torch.int32).to(DEV),
            torch.full((BATCH,), 2, dtype=torch.int32).to(DEV))
    tr.backward()
    torch.cuda.synchronize()


def test_trainer_one_pair_end_to_end(yv, monkeypatch):
    """YOLOv8n, nc 5, 2 x 64 x 64, one state, one batch: the flag-off trainer against a flag-on trainer whose plan is cut down to
    the pair model.2.m.0.cv2 -> model.2.m.0.cv1, so that everything backward() runs before the pair is the same launches.  The
    gradient da the consumer's data gradient stores is bit-equal; the producer's dz, dgamma and dbeta are within the gate of
    test_bnbwd_random_data_silu around the fp64 reference on that da."""
    consumer, producer = PAIR
    off, on = trainer_pair(yv, fused_bn_bwd=False), trainer_pair(yv, fused_bn_bwd=True)
    assert off.bn_bwd_ws is None and not off._bnbwd_of and on._bnbwd_of[consumer] == producer and len(on._bnbwd_of) == 29
    on._bnbwd_of, on._bnbwd_producers = {consumer: producer}, {producer}
    for tr in (off, on):
        run_step(tr)
    po, pn = off.block[producer], on.block[producer]
    T, C = BATCH * off.geom[producer][1] ** 2, po.cout
    da_off, da_on = off.act[po.e.out[0]].grad[:T], on.act[pn.e.out[0]].grad[:T]
    assert da_off.shape[1] == C and bool((da_off != 0).any())
    assert torch.equal(da_off.view(torch.int16), da_on.view(torch.int16)), "da differs between the trainers"
    assert torch.equal(off.z[producer], on.z[producer])
    route = yv.conv_bnbwd_route(BATCH, off.geom[consumer][0], off.geom[consumer][0], 3, 1, off.block[consumer].cout, C)
    consts = [t.cpu() for t in (*pn.stat, *pn.affine)]
    want = fused_reference(monkeypatch, da_on.cpu(), on.z[producer][:T].cpu(), consts, width_of(yv, route.kernel))
    print(f"\n{producer}: T = {T}, C = {C}, instance {route.kernel}")
    gate(on.dz[producer][:T].cpu(), want, "dz")
    gate(pn.daffine[0].cpu(), want, "dgamma"); gate(pn.daffine[1].cpu(), want, "dbeta")


def test_trainer_parameter_gradients_against_the_unfused_trainer(yv):
    """The same step on the flag-off and the flag-on trainer.  A plain block of the head (Detect's last 1 x 1 layers) has the
    loss's own gradient as its output gradient: no fused producer lies behind it in backward(), its gradients are bit-equal.  Every
    other gradient has one (the head's `.1` blocks are fused producers themselves) and is within the per-module tolerance of
    tests/test_gpu_yolo_train.py (relative L2 3e-2).  Measured on the MI355X: the worst is model.2.m.0.cv2.bn.bias at 2.98e-2, deep in
    backward() on 16 x 16 maps of two images, where the differences in the last bit of dz upstream have been amplified the most (the
    note of test_trainer_local_consistency on random-init BatchNorm stacks); the run is bitwise reproducible."""
    from test_gpu_yolo_train import rel_l2
    off, on = trainer_pair(yv, fused_bn_bwd=False), trainer_pair(yv, fused_bn_bwd=True)
    for tr in (off, on):
        run_step(tr)
    g_off, g_on = off.grads(), on.grads()
    plain = {b.key for b in on.blocks if not b.bn}
    assert len(plain) == 6 and set(g_off) == set(g_on)
    worst = ("", 0.0)
    for k in g_off:
        if k.rsplit(".", 1)[0] in plain:
            assert torch.equal(g_off[k], g_on[k]), k
        elif float(g_off[k].norm()) > 0:
            e = rel_l2(g_on[k], g_off[k])
            worst = max(worst, (k, e), key=lambda kv: kv[1])
            assert e < 3e-2, (k, e)
    print(f"\nworst relative L2 of a gradient against the unfused trainer: {worst}")


def test_trainer_fused_bn_bwd_passes_the_trainer_checks(yv, monkeypatch):
    """YV_YOLO_FUSED_BN_BWD=1: the project's own trainer checks (tests/test_gpu_yolo_train.py, their tolerances) pass; bn_act_bwd is
    never called for an eligible producer, and bn_act_bwd_finish runs once per eligible producer and backward pass (1 backward + 12
    training steps)."""
    import yvhip.yolo_training as yt
    from test_gpu_yolo_train import test_trainer_local_consistency, test_training_steps_reduce_the_loss
    monkeypatch.setenv("YV_YOLO_FUSED_BN_BWD", "1")
    probe = yt.YoloTrainer(yt.init_yolo_train_state("n", 5, seed=1), scale="n", nc=5, size=160, batch=2)
    assert probe.fused_bn_bwd is True and len(probe._bnbwd_producers) == 29
    eligible_dz = {probe.dz[k].shape for k in probe._bnbwd_producers}
    del probe
    pairs = set(yt.fused_bn_bwd_pairs("n", 5))
    real_bwd, real_finish, calls = yt.bn_act_bwd, yt.bn_act_bwd_finish, [0]
    seen = []

    def guarded(tr_self, b, da=None, _real=yt.YoloTrainer._bwd):
        seen.append(b.key)
        return _real(tr_self, b, da)

    def no_bwd_for_eligible(*a, **kw):
        assert seen[-1] not in pairs, f"bn_act_bwd called for the eligible producer {seen[-1]}"
        return real_bwd(*a, **kw)

    def counted(*a, **kw):
        assert seen[-1] in pairs
        calls[0] += 1
        return real_finish(*a, **kw)

    monkeypatch.setattr(yt.YoloTrainer, "_bwd", guarded)
    monkeypatch.setattr(yt, "bn_act_bwd", no_bwd_for_eligible)
    monkeypatch.setattr(yt, "bn_act_bwd_finish", counted)
    test_trainer_local_consistency(yv, "n", 5, 160, 2)
    test_training_steps_reduce_the_loss(yv)
    assert calls[0] == 29 * (1 + 12), calls[0]
    assert eligible_dz
