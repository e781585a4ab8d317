"""yv_conv2d_stats + yv_bn_stats_finish (YoloTrainer(fused_bn_stats=True)): the convolution of yv_conv2d_ws that also writes the
per-tile column sums of what it stores, on every kernel route a single-source convolution can take.

Exact cases use the conventions of test_gpu_conv_routes.py (loud borders, a sentinel in every output, the route asserted before it
runs) with operands from {-1, 0, 1} and thinned weights, so that every z is a small integer (exact in bf16) and every column sum
of z and z^2 stays below 2^24: every f32 partial sum, in any order, is then an exact integer, and the comparisons are equalities.
The condition is computed on the CPU reference in int64 and asserted before anything is launched."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_routes import DEV, SENTINEL, Options, bf, case, codes, query

pytestmark = pytest.mark.gpu
EPS, MOMENTUM = 1e-3, 0.03
PAD = 192                       # floats allocated behind yv_conv_stats_ws_floats: must keep the sentinel


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def stats_cases(yv):
    """(case, options).  Notation of the names: B x H x W, k / stride, Cin -> Cout."""
    k = codes(yv)
    I16, I32, I64, I128, D64, D128, S = k["I16"], k["I32"], k["I64"], k["I128"], k["D64"], k["D128"], yv.CONV_STAGED
    return [
        (case("igemm16", 2, 10, 12, 3, 1, [(32, 0, 0, 0)], 16, I16), {}),
        (case("igemm32_slices_s2", 1, 7, 5, 3, 2, [(24, 0, 8, 40)], 24, I32, out=(8, 40)), {}),
        (case("igemm64_staged_s2", 2, 11, 9, 3, 2, [(48, 0, 0, 0)], 64, I64), {}),
        (case("igemm64_direct_c_off4", 2, 10, 10, 3, 1, [(64, 0, 0, 0)], 64, k["I64_DIRECT"], out=(4, 72), query=D64), {}),
        (case("igemm128_ragged_n", 2, 17, 9, 3, 1, [(32, 0, 0, 0)], 96, I128), {}),
        (case("igemm128_n144", 1, 13, 13, 1, 1, [(96, 0, 0, 0)], 144, I128), {}),
        (case("dma64_1x1_nk1", 2, 13, 13, 1, 1, [(64, 0, 0, 0)], 64, D64), {}),
        (case("dma64_1x1_nk2_n80", 2, 9, 15, 1, 1, [(128, 0, 0, 0)], 80, D64), {}),
        (case("dma64_3x3_cin576_n192", 1, 10, 10, 3, 1, [(576, 0, 0, 0)], 192, D64), {}),
        (case("dma64_stride2", 2, 10, 9, 3, 2, [(64, 0, 0, 0)], 80, D64), {}),
        (case("dma64_T5_one_ragged_tile", 5, 1, 1, 3, 1, [(64, 0, 0, 0)], 64, D64), {}),
        (case("dma64_T1122_nine_tiles", 2, 33, 17, 3, 1, [(192, 0, 0, 0)], 144, D64), {}),
        (case("dma128_320x320_n80", 1, 320, 320, 1, 1, [(64, 0, 0, 0)], 80, D128), {}),
        (case("fold_T266240_2080_tiles", 1, 512, 520, 1, 1, [(64, 0, 0, 0)], 80, D128), {}),
        (case("dma64_two_stage", 2, 20, 20, 3, 1, [(64, 0, 0, 0)], 64, yv.CONV_DMA_64_2 | S), dict(conv_dma=1)),
        (case("dma128_three_stage", 2, 20, 20, 3, 1, [(128, 0, 0, 0)], 128, yv.CONV_DMA_128_3 | S), dict(conv_dma=3)),
        (case("dma64_four_stage", 2, 20, 20, 3, 1, [(128, 0, 0, 0)], 128, yv.CONV_DMA_64_4 | S), dict(conv_dma=4)),
    ]


def case_names():
    import yvhip
    return [c["name"] for c, _ in stats_cases(yvhip)]


def find(yv, name):
    return next((c, o) for c, o in stats_cases(yv) if c["name"] == name)


def tiles_of(T):
    return (T + 127) // 128


def tile_sums(v):
    """(T, C) -> (tiles, C): the sum over each tile of 128 rows (the last one ragged), in v's dtype."""
    T, C = v.shape
    n = tiles_of(T)
    p = torch.zeros((n * 128, C), dtype=v.dtype)
    p[:T] = v
    return p.view(n, 128, C).sum(1)


def make_int_data(c, seed):
    """Operands from {-1, 0, 1} (loud borders as in test_gpu_conv_routes), weights thinned to one nonzero in four (one in sixteen
    for K = 5184), a bias from {-1, 0, 1}; the exact reference z in int64 and the integer-exactness condition asserted on it."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, k, s = c["B"], c["H"], c["W"], c["k"], c["s"]
    (ch, _, off, ld), = c["srcs"]
    x = torch.randint(-1, 2, (B, H * s, W * s, ld), generator=g).float()
    x[:, 0] = 1; x[:, :, 0] = 1; x[:, -1] = -1; x[:, :, -1] = -1
    K = k * k * ch
    wk = torch.randint(-1, 2, (c["cout"], k, k, ch), generator=g).float()
    wk = wk * (torch.randint(0, 16 if K == 5184 else 4, wk.shape, generator=g) == 0)
    bias = torch.randint(-1, 2, (c["cout"],), generator=g).float()
    xin = x[..., off:off + ch].permute(0, 3, 1, 2).contiguous()
    lin = F.conv2d(xin, wk.permute(0, 3, 1, 2).contiguous(), None, stride=s, padding=k // 2)       # |sums| <= K < 2^24: exact in fp32
    z = (lin.permute(0, 2, 3, 1).contiguous() + bias).reshape(B * H * W, c["cout"])
    zi = z.to(torch.int64)
    assert torch.equal(zi.float(), z)
    # the condition: every z exact in bf16, every column sum of z^2 (hence of |z|) below 2^24
    assert int(zi.abs().max()) <= 256, int(zi.abs().max())
    ratio = int((zi * zi).sum(0).max()) / 2 ** 24
    assert ratio < 1.0, ratio
    return dict(x=x, w=wk.reshape(c["cout"], K), bias=bias, z=zi, ratio=ratio)


def run_stats(yv, c, d, flags=0, ws_floats=None, with_bias=True):
    """conv_view_stats of the case into sentinel-filled buffers; returns (whole out buffer, whole stats_ws, need)."""
    T = c["B"] * c["H"] * c["W"]
    need = yv.conv_stats_ws_floats(T, c["cout"])
    out = torch.full((c["B"], c["H"], c["W"], c["out"][1]), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((need + PAD if ws_floats is None else ws_floats,), SENTINEL, device=DEV)
    (ch, up, off, _), = c["srcs"]
    yv.conv_view_stats(yv.view(d["x_d"], off, ch, up), c["B"], c["H"], c["W"], c["k"], c["s"], d["w_d"], c["cout"],
                       yv.mview(out, c["out"][0], c["cout"]), ws, bias=d["bias_d"] if with_bias else None, flags=flags)
    torch.cuda.synchronize()
    return out, ws, need


def run_plain(yv, c, d):
    out = torch.full((c["B"], c["H"], c["W"], c["out"][1]), SENTINEL, dtype=torch.bfloat16, device=DEV)
    (ch, up, off, _), = c["srcs"]
    yv.conv_view(yv.view(d["x_d"], off, ch, up), c["B"], c["H"], c["W"], c["k"], c["s"], d["w_d"], c["cout"],
                 yv.mview(out, c["out"][0], c["cout"]), bias=d["bias_d"])
    torch.cuda.synchronize()
    return out


def to_dev(d):
    d["x_d"], d["w_d"], d["bias_d"] = bf(d["x"]).to(DEV), bf(d["w"]).to(DEV), d["bias"].to(DEV)
    return d


def finish(yv, ws, T, C, run_mean0, run_var0):
    mean, rstd = torch.full((C,), SENTINEL, device=DEV), torch.full((C,), SENTINEL, device=DEV)
    rm, rv = run_mean0.clone(), run_var0.clone()
    yv.bn_stats_finish(ws, T, mean, rstd, rm, rv, EPS, MOMENTUM)
    torch.cuda.synchronize()
    return mean, rstd, rm, rv


def running_init(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", case_names())
def test_conv_stats_exact_integer(yv, name):
    """Every route: `out` is the exact integer reference and what conv_view writes, bit for bit; the channels outside the slice
    and the floats behind yv_conv_stats_ws_floats keep the sentinel; every tile partial equals the exact sum over that tile's
    rows (so a value credited to the wrong tile, or counted twice, shows even where the totals agree) and the totals equal the
    int64 column sums; bn_stats_finish gives the bits bn_stats gives on the stored z from the same running estimates."""
    c, opts = find(yv, name)
    d = to_dev(make_int_data(c, seed=sum(map(ord, name))))
    T, C = c["B"] * c["H"] * c["W"], c["cout"]
    off = c["out"][0]
    print(f"\n{name}: T = {T}, {tiles_of(T)} tiles, max column sum of z^2 / 2^24 = {d['ratio']:.3f}")
    with Options(yv, **opts):
        assert query(yv, c, yv.EPI_BIAS) == c["query"], name
        out, ws, need = run_stats(yv, c, d)
        plain = run_plain(yv, c, d)
    got = out[..., off:off + C].reshape(T, C)
    assert torch.equal(got.cpu(), bf(d["z"].float())), "out differs from the integer reference"
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), "out differs from conv_view's"
    outside = torch.cat([out[..., :off], out[..., off + C:]], -1)
    assert bool((outside == SENTINEL).all()), "wrote outside its channels"
    n = tiles_of(T)
    assert need >= n * 2 * C
    assert bool((ws[need:] == SENTINEL).all()), "wrote behind yv_conv_stats_ws_floats"
    part = ws[:n * 2 * C].view(n, 2, C).cpu().double()
    z = d["z"]
    assert torch.equal(part[:, 0], tile_sums(z).double()), "a tile's sum"
    assert torch.equal(part[:, 1], tile_sums(z * z).double()), "a tile's sum of squares"
    assert torch.equal(part[:, 0].sum(0), z.sum(0).double()) and torch.equal(part[:, 1].sum(0), (z * z).sum(0).double())
    # the finaliser against bn_stats on the stored z (a dense copy: bn_stats wants a 16-byte aligned view)
    rm0, rv0 = running_init(C, 7)
    mean, rstd, rm, rv = finish(yv, ws, T, C, rm0, rv0)
    assert bool((ws[need:] == SENTINEL).all()), "bn_stats_finish wrote behind yv_conv_stats_ws_floats"
    zs = got.contiguous()
    mean2, rstd2 = torch.full((C,), SENTINEL, device=DEV), torch.full((C,), SENTINEL, device=DEV)
    rm2, rv2 = rm0.clone(), rv0.clone()
    yv.bn_stats(yv.mview(zs), T, mean2, rstd2, rm2, rv2, torch.zeros(yv.bn_ws_floats(T, C), device=DEV), EPS, MOMENTUM)
    torch.cuda.synchronize()
    for a, b, what in ((mean, mean2, "mean"), (rstd, rstd2, "rstd"), (rm, rm2, "run_mean"), (rv, rv2, "run_var")):
        assert torch.equal(a, b), what
    assert not torch.equal(rm, rm0) and not torch.equal(rv, rv0)


# ------------------------------------------------------------------------------------------------ 2
def partial_bounds(v):
    """v (T, C) float64, the stored z.  A tile partial is an f32 sum of at most 128 values: in any order it errs by at most
    128 * 2^-24 * (sum over the tile's rows of |v|), with v^2 for the sum of squares (the rounding of each square included: 127
    additions + 1 product), times 1.01 for the higher-order terms."""
    u = 1.01 * 128 * 2.0 ** -24
    return tile_sums(v), tile_sums(v * v), u * tile_sums(v.abs()), u * tile_sums(v * v)


def stats_from_partials(part, T):
    """The finaliser's formulas in float64: m = s / T, var = max(ss / T - m^2, 0), rstd = 1 / sqrt(var + eps)."""
    s, ss = part[:, 0].sum(0), part[:, 1].sum(0)
    m = s / T
    var = (ss / T - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + EPS)


def ulp32(x):
    x32 = x.float()
    return (torch.nextafter(x32.abs(), torch.full_like(x32, math.inf)) - x32.abs()).double()


@pytest.mark.parametrize("name", ["igemm64_direct_c_off4", "dma64_T1122_nine_tiles"])
def test_conv_stats_random_data(yv, name):
    """randn inputs, randn / sqrt(K) weights, no bias.  Reference: float64 over the STORED z.  Every (tile, channel) partial
    within partial_bounds; mean and rstd of bn_stats_finish within 1 ulp of f32 of the finaliser's formulas evaluated in float64
    on the partials read back (both sum in double, in a different order); two calls give the same bits."""
    c, opts = find(yv, name)
    g = torch.Generator().manual_seed(len(name))
    (ch, _, _, ld), = c["srcs"]
    K = c["k"] ** 2 * ch
    T, C, off = c["B"] * c["H"] * c["W"], c["cout"], c["out"][0]
    d = dict(x=torch.randn(c["B"], c["H"] * c["s"], c["W"] * c["s"], ld, generator=g),
             w=torch.randn(C, K, generator=g) / math.sqrt(K), bias=torch.zeros(C))
    to_dev(d)
    n = tiles_of(T)
    runs = []
    with Options(yv, **opts):
        assert query(yv, c, 0) == c["query"], name
        for _ in range(2):
            out, ws, need = run_stats(yv, c, d, with_bias=False)
            rm0, rv0 = running_init(C, 9)
            runs.append((out, ws, finish(yv, ws, T, C, rm0, rv0)))
    (out, ws, st), (out_b, ws_b, st_b) = runs
    assert torch.equal(out.view(torch.int16), out_b.view(torch.int16)) and torch.equal(ws[:need], ws_b[:need])
    assert all(torch.equal(a, b) for a, b in zip(st, st_b))
    v = out[..., off:off + C].reshape(T, C).cpu().double()
    part = ws[:n * 2 * C].view(n, 2, C).cpu().double()
    s_ref, q_ref, s_bound, q_bound = partial_bounds(v)
    es, eq = (part[:, 0] - s_ref).abs(), (part[:, 1] - q_ref).abs()
    print(f"\n{name}: worst partial error / bound: sum {float((es / s_bound).max()):.3f}, squares {float((eq / q_bound).max()):.3f}")
    assert bool((es <= s_bound).all()) and bool((eq <= q_bound).all())
    m, r = stats_from_partials(part, T)
    mean, rstd = st[0].cpu().double(), st[1].cpu().double()
    assert bool(((mean - m).abs() <= ulp32(m)).all()), float(((mean - m).abs() / ulp32(m)).max())
    assert bool(((rstd - r).abs() <= ulp32(r)).all()), float(((rstd - r).abs() / ulp32(r)).max())


# ------------------------------------------------------------------------------------------------ 3
def test_conv_stats_rejects(yv):
    """The argument checks of tests/test_conv_stats_cpu.py with real tensors: a forbidden flag and a short workspace raise and
    leave `out` and `stats_ws` untouched."""
    c, _ = find(yv, "dma64_1x1_nk2_n80")
    d = to_dev(make_int_data(c, seed=3))
    T = c["B"] * c["H"] * c["W"]
    need = yv.conv_stats_ws_floats(T, c["cout"])
    out = torch.full((c["B"], c["H"], c["W"], c["cout"]), SENTINEL, dtype=torch.bfloat16, device=DEV)

    def call(ws, flags):
        (ch, up, off, _), = c["srcs"]
        yv.conv_view_stats(yv.view(d["x_d"], off, ch, up), c["B"], c["H"], c["W"], c["k"], c["s"], d["w_d"], c["cout"], yv.mview(out),
                           ws, bias=d["bias_d"], flags=flags)

    with Options(yv):
        for flags, floats in ((yv.EPI_SILU, need), (yv.EPI_RES_BF16, need), (yv.EPI_OUT_F32, need), (yv.EPI_GELU, need),
                              (0, need - 1), (0, tiles_of(T) * 2 * c["cout"] - 8)):
            ws = torch.full((floats,), SENTINEL, device=DEV)
            with pytest.raises(yv.YvError):
                call(ws, flags)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all()), (flags, floats)
        ws = torch.full((need,), SENTINEL, device=DEV)                  # the same call with nothing wrong runs
        call(ws, 0)
        torch.cuda.synchronize()
        assert not bool((out == SENTINEL).any()) and not bool((ws == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ 4
def test_trainer_fused_bn_stats_first_layer(yv):
    """Two YoloTrainers ("n", nc 5, 2 x 160 x 160) from one state on one batch, fused_bn_stats off and on.  The stem convolution
    has the same input in both: its z must be equal, and its batch statistics must both lie within the summation bound of
    test_conv_stats_random_data around the float64 statistics of that z.  The bound n * 2^-24 * sum |v| * 1.01 is that of an f32
    sum of n values in any order: n = 128 (a tile) for the fused path, n = 256 for bn_stats, whose chunks are 256 rows at T = 12,800
    (chunks_for: ceil(T / 256) = 50 chunks); the sums of the partials are in double in both.  Carried to the statistics:
    |dm| <= E_s / T, |dvar| <= E_q / T + 2 |m| E_s / T + (E_s / T)^2, |drstd| <= rstd^3 / 2 * |dvar| (first order, times 1.01), plus one
    f32 rounding of the result."""
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    scale, nc, S, B = "n", 5, 160, 2
    sd = init_yolo_train_state(scale, nc, seed=3)
    img = torch.randint(0, 256, (B, S, S, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).to(DEV)
    trs = {}
    for fused in (False, True):
        tr = YoloTrainer({k: v.clone() for k, v in sd.items()}, scale=scale, nc=nc, size=S, batch=B, fused_bn_stats=fused)
        assert tr.fused_bn_stats is fused
        keys = [b.key for b in tr.blocks if b.bn]
        init = {k: (tr.run_mean[k].clone(), tr.run_var[k].clone()) for k in keys}
        tr.forward(img)
        torch.cuda.synchronize()
        for k in keys:
            assert bool((tr.run_mean[k] != init[k][0]).any()) and bool((tr.run_var[k] != init[k][1]).any()), (fused, k)
        trs[fused] = tr
    key = trs[False].blocks[0].key
    hin, hout = trs[False].geom[key]
    T = B * hout * hout
    assert hin == S and T == 12800
    z = trs[False].z[key][:T]
    assert torch.equal(z, trs[True].z[key][:T])
    v = z.cpu().double()
    m = v.mean(0)
    var = ((v * v).mean(0) - m * m).clamp_min(0.0)
    r = 1.0 / torch.sqrt(var + EPS)
    for fused, rows in ((True, 128), (False, 256)):
        u = 1.01 * rows * 2.0 ** -24
        dm = u * v.abs().sum(0) / T
        dvar = u * (v * v).sum(0) / T + 2 * m.abs() * dm + dm * dm
        dr = 1.01 * 0.5 * r ** 3 * dvar
        mean, rstd = trs[fused].mean[key].cpu().double(), trs[fused].rstd[key].cpu().double()
        print(f"\nfused {fused}: mean error / bound {float(((mean - m).abs() / (dm + ulp32(m))).max()):.3f}, "
              f"rstd error / bound {float(((rstd - r).abs() / (dr + ulp32(r))).max()):.3f}")
        assert bool(((mean - m).abs() <= dm + ulp32(m)).all()), fused
        assert bool(((rstd - r).abs() <= dr + ulp32(r)).all()), fused


# ------------------------------------------------------------------------------------------------ 5
def test_trainer_fused_bn_stats_passes_the_trainer_checks(yv, monkeypatch):
    """YV_YOLO_FUSED_BN_STATS=1: the project's own trainer checks (tests/test_gpu_yolo_train.py, their tolerances: outputs 6e-3,
    gradients 3e-2, the loss comes down) pass with the fused statistics, the default bn_stats is never called, and
    conv_view_stats runs once per BatchNorm block and forward pass (1 forward + 12 training steps)."""
    import yvhip.yolo_training as yt
    from test_gpu_yolo_train import test_trainer_local_consistency, test_training_steps_reduce_the_loss
    monkeypatch.setenv("YV_YOLO_FUSED_BN_STATS", "1")
    probe = yt.YoloTrainer(yt.init_yolo_train_state("n", 5, seed=1), scale="n", nc=5, size=160, batch=2)
    assert probe.fused_bn_stats is True
    n_bn = sum(1 for b in probe.blocks if b.bn)
    assert n_bn > 50
    del probe

    def no_bn_stats(*a, **kw):
        raise AssertionError("bn_stats called with YV_YOLO_FUSED_BN_STATS=1")

    calls = [0]
    real = yt.conv_view_stats

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(yt, "bn_stats", no_bn_stats)
    monkeypatch.setattr(yt, "conv_view_stats", counted)
    test_trainer_local_consistency(yv, "n", 5, 160, 2)
    test_training_steps_reduce_the_loss(yv)
    assert calls[0] == n_bn * (1 + 12), (calls[0], n_bn)
