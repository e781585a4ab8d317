"""The grouped convolution launch (yv_conv2d_group: cgemm_dma_group_kernel<64, 4, 1, 3>, cgemm_small_group_kernel<64, 2> and <32, 4>)
against the exact integer reference of tests/test_gpu_conv_routes.py and, bit for bit, against each member's own single launch.

Integer operands in [-1, 1] with loud borders in every channel of the buffer, outputs prefilled with 0.5, torch.equal against
F.conv2d in fp32; |y| < 256 is asserted, where bf16 holds every integer, so the staged epilogue's two roundings of a shortcut and
the direct epilogue's one give the same exact integer (tests/test_gpu_conv_small.py).  Every test asserts the plan
(yvhip.conv2d_group_plan: the partition function the launch uses) before it launches."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_routes import DEV, SENTINEL, Options, bf, case, expected, kind_flags, launch, make_data, split_out, to_device
from test_gpu_conv_small import CASES as SMALL_CASES, ON

pytestmark = pytest.mark.gpu
INSTANCES = ("dma64", "small64", "small32")


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def inst_options(inst):
    """Options under which every eligible member takes the instance, its code, and its tile rows."""
    if inst == "dma64":
        return dict(conv_small=0), 128
    rows = 64 if inst == "small64" else 32
    return dict(conv_small_rows=rows, **ON), rows


def inst_code(yv, inst):
    return {"dma64": yv.CONV_DMA_64_3 | yv.CONV_STAGED, "small64": yv.CONV_SMALL_64, "small32": yv.CONV_SMALL_32}[inst]


def group_cases(inst):
    """Five members of different shape (the shapes of test_gpu_conv_small.py) and one whose workgroups number more than 8 and no
    multiple of 8; it is a 1 x 1 (one K step per tile), so that heavier members lie in front of it and its remap runs with a
    non-zero remainder at a non-zero first workgroup."""
    big = case("big_23x23x2_n64", 2, 23, 23, 1, 1, [(64, 0, 0, 0)], 64, 0) if inst == "dma64" else \
        case("big_17x17_n128", 1, 17, 17, 1, 1, [(64, 0, 0, 0)], 128, 0)
    return [dict(SMALL_CASES["m35_3x3_cin64"]), dict(SMALL_CASES["m35_1x1_nk1"]), dict(SMALL_CASES["m81_3x3_cin128_n128"]),
            case("m162_3x3_stride2_n72", 2, 9, 9, 3, 2, [(64, 0, 0, 0)], 72, 0), dict(SMALL_CASES["m80_two_src_64up_64"]), big]


def shape_of(yv, c, flags):
    c1 = c["srcs"][1][0] if len(c["srcs"]) > 1 else 0
    return (c["B"], c["H"], c["W"], c["k"], c["s"], c["srcs"][0][0], c1, c["cout"], c["out"][1],
            c["res"][1] if flags & yv.EPI_RES_BF16 else 0, flags)


def fresh_out(yv, c, flags):
    f32 = bool(flags & yv.EPI_OUT_F32)
    return torch.full((c["B"], c["H"], c["W"], c["out"][1]), SENTINEL, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)


def member(yv, c, d, flags, out=None):
    """conv2d's argument list for the case, as conv2d_group takes it; returns (member, output buffer)."""
    out = fresh_out(yv, c, flags) if out is None else out
    views = [yv.view(t, off, ch, up) for t, (ch, up, off, _) in zip(d["bufs_d"], c["srcs"])]
    has_res = bool(flags & yv.EPI_RES_BF16)
    return (views[0], views[1] if len(views) > 1 else None, c["B"], c["H"], c["W"], c["k"], c["s"], d["w_d"], d["bias_d"], out,
            c["out"][0], flags, d["res_d"] if has_res else None, c["res"][0] if has_res else 0), out


def run_group(yv, cs, ds, flags, outs=None):
    ms = [member(yv, c, d, flags, None if outs is None else o) for c, d, o in zip(cs, ds, outs or [None] * len(cs))]
    yv.conv2d_group([m for m, _ in ms])
    torch.cuda.synchronize()
    return [o for _, o in ms]


def assert_exact(yv, c, d, out, kind, staged, what):
    got, outside = split_out(c, out)
    exp = expected(c, d, kind, staged).to(DEV)
    assert bool((outside == SENTINEL).all()), (c["name"], kind, what, "wrote outside its channels")
    if not torch.equal(got, exp):
        bad = (got.float() != exp.float()).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{c['name']} {kind} {what}: {len(bad)} of {got.numel()} values differ, first at (b, y, x, n) = {i}: "
                             f"got {float(got[i])}, expected {float(exp[i])}")


def data(c, seed):
    d = to_device(c, make_data(c, seed=seed, amp=1, wamp=1, ramp=64))
    assert float(d["ref"].abs().max()) < 256
    return d


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("kind", ("bf16", "f32", "res"))
@pytest.mark.parametrize("inst", INSTANCES)
def test_exact_integer_parity(yv, inst, kind):
    """Six members of different shape in ONE launch of the instance: each equals the integer reference and, buffer for buffer (the
    sentinel outside its channels included), its own single launch."""
    opts, rows = inst_options(inst)
    cs = group_cases(inst)
    ds = [data(c, seed=sum(map(ord, c["name"]))) for c in cs]
    fl = kind_flags(yv, kind)
    code = inst_code(yv, inst)
    with Options(yv, **opts):
        n, plan = yv.conv2d_group_plan([shape_of(yv, c, fl) for c in cs])
        assert n == 1 and all(p["launch"] == 0 and p["instance"] == code for p in plan), plan
        big = plan[-1]
        nwg = -(-cs[-1]["B"] * cs[-1]["H"] * cs[-1]["W"] // rows) * -(-cs[-1]["cout"] // 64)
        assert nwg > 8 and nwg % 8 != 0 and big["first_wg"] > 0 and big["first_wg"] % 8 == 0, (nwg, big)
        outs = run_group(yv, cs, ds, fl)
        singles = [launch(yv, c, d, fl) for c, d in zip(cs, ds)]
    for c, d, out, single in zip(cs, ds, outs, singles):
        assert_exact(yv, c, d, out, kind, bool(code & yv.CONV_STAGED), inst)
        assert torch.equal(out, single), (c["name"], kind, inst, "differs from its single launch")


# ------------------------------------------------------------------------------------------------ 6
def reref(c, d):
    """d["ref"] recomputed from d["bufs"], d["w"], d["bias"] (make_data's reference; one source, no upsample)."""
    ch, _, off, _ = c["srcs"][0]
    x = d["bufs"][0][..., off:off + ch].permute(0, 3, 1, 2).contiguous()
    w = d["w"].reshape(c["cout"], c["k"], c["k"], ch).permute(0, 3, 1, 2).contiguous()
    d["ref"] = F.conv2d(x, w, None, stride=c["s"], padding=c["k"] // 2).permute(0, 2, 3, 1).contiguous() + d["bias"]
    assert float(d["ref"].abs().max()) < 256
    return d


@pytest.mark.parametrize("inst", INSTANCES)
def test_two_members_on_slices_of_one_source_and_one_output(yv, inst):
    """The head's own form: channels [0, 64) and [64, 128) of ONE source buffer into channels [0, 64) and [64, 128) of ONE output
    buffer (9 x 9, 3 x 3).  Each slice is exact; with the other member absent the other slice keeps the sentinel."""
    opts, _ = inst_options(inst)
    ca = case("slice_a", 1, 9, 9, 3, 1, [(64, 0, 0, 128)], 64, 0, out=(0, 128))
    cb = case("slice_b", 1, 9, 9, 3, 1, [(64, 0, 64, 128)], 64, 0, out=(64, 128))
    da, db = make_data(ca, seed=21, amp=1, wamp=1), make_data(cb, seed=22, amp=1, wamp=1)
    db["bufs"] = da["bufs"]                                            # one source buffer
    da, db = to_device(ca, reref(ca, da)), to_device(cb, reref(cb, db))
    db["bufs_d"] = da["bufs_d"]
    code = inst_code(yv, inst)
    with Options(yv, **opts):
        n, plan = yv.conv2d_group_plan([shape_of(yv, ca, 0), shape_of(yv, cb, 0)])
        assert n == 1 and [p["instance"] for p in plan] == [code, code]
        out = fresh_out(yv, ca, 0)
        run_group(yv, [ca, cb], [da, db], 0, outs=[out, out])
        only_a, only_b = fresh_out(yv, ca, 0), fresh_out(yv, ca, 0)
        run_group(yv, [ca], [da], 0, outs=[only_a])
        run_group(yv, [cb], [db], 0, outs=[only_b])
    ea, eb = bf(da["ref"]).to(DEV), bf(db["ref"]).to(DEV)
    assert torch.equal(out[..., :64], ea) and torch.equal(out[..., 64:], eb)
    assert torch.equal(only_a[..., :64], ea) and bool((only_a[..., 64:] == SENTINEL).all())
    assert torch.equal(only_b[..., 64:], eb) and bool((only_b[..., :64] == SENTINEL).all())
    assert not torch.equal(ea, eb)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("inst", INSTANCES)
def test_members_of_one_shape_keep_their_own_operands(yv, inst):
    opts, _ = inst_options(inst)
    cs = [dict(SMALL_CASES["m35_3x3_cin64"]) for _ in range(3)]
    ds = [data(c, seed=100 + i) for i, c in enumerate(cs)]
    assert not torch.equal(ds[0]["ref"], ds[1]["ref"]) and not torch.equal(ds[1]["ref"], ds[2]["ref"])
    with Options(yv, **opts):
        n, plan = yv.conv2d_group_plan([shape_of(yv, c, 0) for c in cs])
        assert n == 1 and [p["position"] for p in plan] == [0, 1, 2]
        outs = run_group(yv, cs, ds, 0)
    for i, (c, d, out) in enumerate(zip(cs, ds, outs)):
        assert_exact(yv, c, d, out, "bf16", False, f"{inst} member {i}")


# ------------------------------------------------------------------------------------------------ 8
def test_partitions_and_leftovers(yv):
    """One call: two members on 32-pixel tiles, two on 64-pixel tiles (128 tiles of 64 pixels: the rule's other side) and one on
    igemm_kernel - three launches, as planned, everything exact.  A group of one; nine members (8 + 1)."""
    small = [dict(SMALL_CASES["m35_3x3_cin64"]), dict(SMALL_CASES["m81_3x3_cin128_n128"])]
    wide = [case(f"m4096_1x1_n128_{i}", 1, 64, 64, 1, 1, [(64, 0, 0, 0)], 128, 0) for i in range(2)]
    ig = case("igemm32_cin24", 2, 9, 11, 3, 1, [(24, 0, 0, 0)], 32, 0)
    cs = [small[0], wide[0], ig, small[1], wide[1]]
    ds = [data(c, seed=40 + i) for i, c in enumerate(cs)]
    with Options(yv, conv_small_rows=0, **ON):
        n, plan = yv.conv2d_group_plan([shape_of(yv, c, 0) for c in cs])
        assert [p["instance"] for p in plan] == [yv.CONV_SMALL_32, yv.CONV_SMALL_64, yv.CONV_IGEMM_32, yv.CONV_SMALL_32, yv.CONV_SMALL_64]
        assert n == 3 and [p["launch"] for p in plan] == [1, 0, 2, 1, 0], plan
        outs = run_group(yv, cs, ds, 0)
        for c, d, out in zip(cs, ds, outs):
            assert_exact(yv, c, d, out, "bf16", False, "mixed call")
    with Options(yv, conv_small=0):
        c, d = small[0], ds[0]
        assert yv.conv2d_group_plan([shape_of(yv, c, 0)])[0] == 1
        assert_exact(yv, c, d, run_group(yv, [c], [d], 0)[0], "bf16", True, "group of one")
        nine = [dict(SMALL_CASES["m35_1x1_nk1"]) for _ in range(9)]
        nd = [data(c, seed=60 + i) for i, c in enumerate(nine)]
        n, plan = yv.conv2d_group_plan([shape_of(yv, c, 0) for c in nine])
        assert n == 2 and [p["launch"] for p in plan] == [0] * 8 + [1]
        for i, (c, d, out) in enumerate(zip(nine, nd, run_group(yv, nine, nd, 0))):
            assert_exact(yv, c, d, out, "bf16", True, f"nine members, member {i}")


def test_rejected_calls_launch_nothing(yv):
    c = dict(SMALL_CASES["m35_3x3_cin64"])
    d = data(c, seed=7)
    with Options(yv, conv_small=0):
        with pytest.raises(yv.YvError):
            yv.conv2d_group([])
        a, out_a = member(yv, c, d, 0)
        b, _ = member(yv, c, d, 0, out=out_a)                          # the same output pointer
        other, out_o = member(yv, c, d, 0)
        with pytest.raises(yv.YvError):
            yv.conv2d_group([other, a, b])
        bad = list(member(yv, c, d, 0)[0])
        bad[5] = 5                                                     # ksize 5: the LAST member is rejected, the first did not run
        first, out_f = member(yv, c, d, 0)
        with pytest.raises(yv.YvError):
            yv.conv2d_group([first, tuple(bad)])
        torch.cuda.synchronize()
    for out in (out_a, out_o, out_f, bad[9]):
        assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("inst", INSTANCES)
def test_silu_equals_the_single_launches_bit_for_bit(yv, inst):
    """bias -> SiLU -> bf16 and -> f32 on integer operands scaled by 1 / 16 (exact pre-activations), as
    test_silu_equals_the_128_row_route_bit_for_bit: the grouped launch runs the member's own instance, so the bits are its."""
    opts, _ = inst_options(inst)
    cs = [dict(SMALL_CASES[n]) for n in ("m81_3x3_cin128_n128", "m70_3x3_cin64_n72", "m80_two_src_slices", "m35_1x1_nk1")]
    ds = []
    for c in cs:
        d = make_data(c, seed=len(c["name"]))
        d["w"], d["bias"] = d["w"] / 16, d["bias"] / 16
        ds.append(to_device(c, d))
    code = inst_code(yv, inst)
    for fl in (yv.EPI_SILU, yv.EPI_SILU | yv.EPI_OUT_F32):
        with Options(yv, **opts):
            n, plan = yv.conv2d_group_plan([shape_of(yv, c, fl) for c in cs])
            assert n == 1 and all(p["instance"] == code for p in plan), plan
            outs = run_group(yv, cs, ds, fl)
            singles = [launch(yv, c, d, fl) for c, d in zip(cs, ds)]
        for c, out, single in zip(cs, outs, singles):
            assert torch.equal(out, single), (c["name"], inst, fl)
            got, outside = split_out(c, out)
            assert bool((outside == SENTINEL).all()) and not bool((got == SENTINEL).all()), (c["name"], inst, fl)


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("inst", INSTANCES)
def test_the_launch_does_not_change_the_result(yv, inst):
    opts, _ = inst_options(inst)
    g = torch.Generator().manual_seed(3)
    cs = [dict(SMALL_CASES["m81_3x3_cin128_n128"]), dict(SMALL_CASES["m35_3x3_cin64"]), dict(SMALL_CASES["m70_1x1_nk2_n128"])]
    ds = []
    for c in cs:
        cin, k = c["srcs"][0][0], c["k"]
        ds.append(dict(bufs_d=[bf(torch.randn(c["B"], c["H"], c["W"], cin, generator=g)).to(DEV)],
                       w_d=bf(torch.randn(c["cout"], k * k * cin, generator=g) * 0.03).to(DEV),
                       bias_d=torch.randn(c["cout"], generator=g).to(DEV), res_d=None))
    with Options(yv, **opts):
        assert yv.conv2d_group_plan([shape_of(yv, c, 0) for c in cs])[0] == 1
        a, b = run_group(yv, cs, ds, 0), run_group(yv, cs, ds, 0)
        singles = [launch(yv, c, d, 0) for c, d in zip(cs, ds)]
    for x, y, s in zip(a, b, singles):
        assert torch.equal(x, y) and torch.equal(x, s)


# ------------------------------------------------------------------------------------------------ 11
def images(B, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, *hw, 3), generator=g, dtype=torch.uint8).to(DEV)


def assert_engines_agree(on, off, sizes=((64, 64), (64, 96)), batches=(1, 2)):
    for hw in sizes:
        a, b = on.resized(hw), off.resized(hw)
        assert a.grouped_head and not b.grouped_head and a.small_maps == b.small_maps
        for B in batches:
            x = images(B, hw, seed=B + hw[1])
            for got, want in zip(a(x), b(x)):
                assert torch.equal(got, want), (hw, B)
            ra, rb = a.forward_raw(x), b.forward_raw(x)
            flat_a, flat_b = [t for part in ra for t in part], [t for part in rb for t in part]
            assert len(flat_a) == len(flat_b) == 6
            for got, want in zip(flat_a, flat_b):
                assert torch.equal(got, want), (hw, B)
                assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0


@pytest.mark.parametrize("small_maps", (False, True))
@pytest.mark.parametrize("nc", (5, 80))
def test_engine_keeps_its_bits(yv, nc, small_maps):
    """YoloEngine(grouped_head=True) against the default engine on the same state: boxes, scores and forward_raw's six tensors,
    B = 1 and 2 at 64 x 64 and 64 x 96.  nc = 80 has no fused tail: the .2 step is a group whose class members are igemm's."""
    from yvhip import engines
    sd = engines.init_yolo_state("n", nc, seed=1, head_gain=4.0)
    on = engines.YoloEngine(sd, "n", nc, 64, DEV, small_maps=small_maps, grouped_head=True)
    off = engines.YoloEngine(sd, "n", nc, 64, DEV, small_maps=small_maps, grouped_head=False)
    assert on.fused_tail == (nc == 5)
    assert_engines_agree(on, off)


def test_mxfp8_engine_keeps_its_bits(yv):
    from yvhip import engines
    sd = engines.init_yolo_state("m", 5, seed=2, head_gain=4.0)
    on = engines.YoloEngine(sd, "m", 5, 64, DEV, dtype="mxfp8", grouped_head=True)
    off = engines.YoloEngine(sd, "m", 5, 64, DEV, dtype="mxfp8", grouped_head=False)
    head = [e for e in engines.detect_launches("m", 5, True, False, True) if type(e) is engines.ConvGroup]
    assert any(c.key in on.wq for g in head for c in g.convs) and any(c.key not in on.wq for g in head for c in g.convs)
    assert_engines_agree(on, off, sizes=((64, 64),))


def test_flag_off_never_calls_the_group(yv, monkeypatch):
    from yvhip import engines

    def boom(members):
        raise AssertionError("conv2d_group called by an engine built with grouped_head=False")
    sd = engines.init_yolo_state("n", 5, seed=1, head_gain=4.0)
    monkeypatch.delenv("YV_YOLO_GROUPED_HEAD", raising=False)
    eng = engines.YoloEngine(sd, "n", 5, 64, DEV)
    assert eng.grouped_head is False and eng.resized((64, 96)).grouped_head is False
    monkeypatch.setattr(engines, "conv2d_group", boom)
    x = images(2, (64, 64), seed=5)
    eng(x)
    eng.forward_raw(x)
    torch.cuda.synchronize()
    monkeypatch.setenv("YV_YOLO_GROUPED_HEAD", "1")
    on = engines.YoloEngine(sd, "n", 5, 64, DEV)
    assert on.grouped_head is True and on.resized((64, 96)).grouped_head is True
    with pytest.raises(AssertionError):
        on(x)
