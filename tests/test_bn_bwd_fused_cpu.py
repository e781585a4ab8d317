"""YoloTrainer(fused_bn_bwd=True) without a GPU: the symbols of yv_conv2d_bnbwd / yv_conv_bnbwd_ws_floats / yv_conv2d_bnbwd_route /
yv_bn_act_bwd_finish, the workspace size rule, every argument check (each is decided on the host before any HIP call, so the
pointers are host addresses that are never dereferenced), the route's `use`, the set of fused pairs and where they stand in
backward(), and the trainer's launches with the flag on, pinned by tests/golden/yolo_bn_bwd_trace.json (written by
`python tests/test_bn_bwd_fused_cpu.py --write`)."""
import ctypes as C
import inspect
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":                              # run as a script: the paths tests/conftest.py sets for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "yolov8-vit_amd")]

import trainer_trace as tt
import yolo_trainer_trace as ytt
import yvhip as yv

ERR_ARG, ERR_LIMIT, ERR_WORKSPACE = -1, -2, -3
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
NEW = ("yv_conv2d_bnbwd", "yv_conv_bnbwd_ws_floats", "yv_conv2d_bnbwd_route", "yv_bn_act_bwd_finish")
WRAPPERS = ("conv_view_bnbwd", "bn_act_bwd_finish", "conv_bnbwd_ws_floats", "conv_bnbwd_route")
FIXTURE = os.path.join(tt.HERE, "golden", "yolo_bn_bwd_trace.json")
FLAG = "YV_YOLO_FUSED_BN_BWD"

# the BatchNorm blocks whose output view exactly one later entry reads, a Block whose input IS that view
ELIGIBLE = sorted(
    ["model.0", "model.1", "model.3", "model.5", "model.7", "model.2.cv2", "model.8.cv2"] +
    [f"model.{i}.m.{j}.cv1" for i, n in ((2, 1), (4, 2), (6, 2), (8, 1), (12, 1), (15, 1), (18, 1), (21, 1)) for j in range(n)] +
    [f"model.22.{cv}.{s}.{b}" for cv in ("cv2", "cv3") for s in range(3) for b in range(2)])
# ... and, at 16 x 640 x 640, the producers the route sends back to conv_view + bn_act_bwd: measured slower (DESIGN.md section 27,
# profiles/bn_bwd_fused_layers.txt) - the consumers' data gradients on 64- / 128-wide instances at >= 100,000 rows, on the 32-wide
# one at >= 400,000 rows with K >= 512
ROUTED_BACK = {
    ("s", 80): {"model.0", "model.1", "model.2.cv2", "model.3", "model.4.m.0.cv1", "model.4.m.1.cv1", "model.15.m.0.cv1",
                "model.22.cv2.0.0", "model.22.cv2.0.1", "model.22.cv3.0.0", "model.22.cv3.0.1"},
    ("n", 5): {"model.2.cv2", "model.3", "model.22.cv2.0.0", "model.22.cv2.0.1", "model.22.cv3.0.0", "model.22.cv3.0.1"},
}


def bnbwd_call(B=2, H=20, W=20, k=3, s=1, cin=64, cout=64, flags=0, ws_floats=None, in_ptr=P, weight=P, out=P, res=None, z=P,
               ldz=None, consts=(P, P, P, P), act=1, stats=P, bias=None, in_ld=None, out_ld=None, res_ld=None):
    """yv_conv2d_bnbwd on dummy pointers; ws_floats None: exactly what yv_conv_bnbwd_ws_floats asks for."""
    v = yv.yv_view(C.c_void_p(in_ptr), in_ld or cin, cin, 0)
    if ws_floats is None:
        ws_floats = yv.conv_bnbwd_ws_floats(B * H * W, cout)
    return yv.lib.yv_conv2d_bnbwd(C.byref(v), B, H, W, k, s, C.c_void_p(weight), C.c_void_p(bias), cout, C.c_void_p(out),
                                  out_ld or cout, C.c_void_p(res), res_ld or cout, flags, C.c_void_p(z), ldz or cout,
                                  *(C.c_void_p(p) for p in consts), act, C.c_void_p(stats), ws_floats, None, 0, None)


# ------------------------------------------------------------------------------------------------ symbols, sizes
def test_symbols_in_header_library_and_bindings():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "yv_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(yv.lib, name), name
        assert name in yv._SIGS and name not in yv.MISSING, name
        assert getattr(yv.lib, name).argtypes == yv._SIGS[name][1], name
    for name in WRAPPERS:
        assert callable(getattr(yv, name)), name
    assert "yv_conv_bnbwd_route_t" in header


@pytest.mark.parametrize("C_", [8, 16, 80, 144])
def test_workspace_floats_both_sides_of_2048_tiles(C_):
    """yv_conv_stats_ws_floats (tile partials, + the fold's chunk partials above 2048 tiles) + the 2 * C coefficients."""
    for T in (1, 5, 127, 128, 129, 1122, 2048 * 128 - 1, 2048 * 128, 2048 * 128 + 1, 266240, 4096 * 128 + 1):
        tiles = -(-T // 128)
        got = yv.conv_bnbwd_ws_floats(T, C_)
        assert got == yv.conv_stats_ws_floats(T, C_) + 2 * C_, (T, C_)
        if tiles <= 2048:
            assert got == tiles * 2 * C_ + 2 * C_, (T, C_)
        else:
            group = -(-tiles // 2048)
            assert got == (tiles + -(-tiles // group)) * 2 * C_ + 2 * C_, (T, C_)
    assert yv.conv_bnbwd_ws_floats(0, C_) == 0 and yv.conv_bnbwd_ws_floats(128, 0) == 0


# ------------------------------------------------------------------------------------------------ argument checks
def test_accepts_the_plain_call_up_to_the_workspace_check():
    """The reference point of the rejections below: the same dummy call with one float too few is rejected for the workspace,
    i.e. it passed every argument check."""
    need = yv.conv_bnbwd_ws_floats(2 * 20 * 20, 64)
    assert bnbwd_call(ws_floats=need - 1) == ERR_WORKSPACE
    assert bnbwd_call(ws_floats=yv.conv_stats_ws_floats(2 * 20 * 20, 64)) == ERR_WORKSPACE          # no room for the coefficients
    assert bnbwd_call(ws_floats=0) == ERR_WORKSPACE
    assert bnbwd_call(flags=yv.EPI_BIAS, bias=P, ws_floats=need - 1) == ERR_WORKSPACE
    assert bnbwd_call(flags=yv.EPI_RES_BF16, res=P, ws_floats=need - 1) == ERR_WORKSPACE
    assert bnbwd_call(flags=yv.EPI_RES_BF16 | yv.EPI_BIAS, res=P, bias=P, act=0, ldz=72, out_ld=80, res_ld=96, ws_floats=need - 1) == ERR_WORKSPACE
    assert bnbwd_call(B=1, H=512, W=520, k=1, cin=64, cout=16, ws_floats=2080 * 2 * 16 + 32) == ERR_WORKSPACE     # no room for the fold


def test_rejects_null_pointers():
    for kw in (dict(in_ptr=None), dict(weight=None), dict(out=None), dict(stats=None), dict(z=None)):
        assert bnbwd_call(**kw) == ERR_ARG, kw
    for i in range(4):
        consts = [P] * 4
        consts[i] = None
        assert bnbwd_call(consts=consts) == ERR_ARG, i
    assert bnbwd_call(flags=yv.EPI_BIAS, bias=None) == ERR_ARG              # a flag without its operand
    assert bnbwd_call(flags=yv.EPI_RES_BF16, res=None) == ERR_ARG


@pytest.mark.parametrize("cout", [4, 12, 20, 60, 68])
def test_rejects_output_channels_that_are_no_multiple_of_8(cout):
    assert bnbwd_call(cout=cout, out_ld=72, ldz=72, ws_floats=1 << 20) == ERR_ARG


@pytest.mark.parametrize("flag", ["EPI_SILU", "EPI_GELU", "EPI_RES_F32", "EPI_OUT_F32", "EPI_POSEMB", "EPI_SAVE_PRE", "EPI_GELU_BWD", 512,
                                  1024, 1 << 30])
def test_rejects_every_flag_but_bias_and_the_bf16_residual(flag):
    f = getattr(yv, flag) if isinstance(flag, str) else flag        # (512: YV_EPI_OUT_MXFP8, internal; above: no flag at all)
    assert bnbwd_call(flags=f, ws_floats=1 << 20) == ERR_ARG
    assert bnbwd_call(flags=f | yv.EPI_BIAS | yv.EPI_RES_BF16, bias=P, res=P, ws_floats=1 << 20) == ERR_ARG


def test_rejects_z_strides_alignment_and_act():
    for ldz in (63, 56, 68, 70):                                     # below Cout, or no multiple of 8
        assert bnbwd_call(ldz=ldz, ws_floats=1 << 20) == ERR_ARG, ldz
    for kw in (dict(z=P + 8), dict(out=P + 8), dict(stats=P + 4), dict(res=P + 8, flags=yv.EPI_RES_BF16),
               dict(consts=(P + 4, P, P, P)), dict(consts=(P, P, P, P + 8)), dict(act=2), dict(act=-1)):
        assert bnbwd_call(ws_floats=1 << 20, **kw) == ERR_ARG, kw


def test_rejects_what_conv2d_rejects_and_sub_batched_sources():
    assert bnbwd_call(k=5, ws_floats=1 << 20) == ERR_ARG
    assert bnbwd_call(s=3, ws_floats=1 << 20) == ERR_ARG
    assert bnbwd_call(cin=12, ws_floats=1 << 20) == ERR_ARG
    # 40 images of 320 x 320 pixels at a pixel stride of 336 channels: beyond 2 GB, yv_conv2d_ws takes it in sub-batches
    assert bnbwd_call(B=40, H=320, W=320, k=1, cin=64, in_ld=336, ws_floats=1 << 30) == ERR_LIMIT


def test_bn_act_bwd_finish_argument_checks():
    f = yv.lib.yv_bn_act_bwd_finish
    p = C.c_void_p(P)
    #     da ldda z  ldz T    C   mean rstd gamma beta act bs dgamma dbeta dz lddz stats_ws stream
    ok = [p, 64, p, 64, 800, 64, p, p, p, p, 1, 1, p, p, p, 64, p, None]
    for i in (0, 2, 6, 7, 8, 9, 12, 13, 14, 16):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_ARG, i
    for i in (0, 2, 14):                                            # da, z, dz: 16-byte aligned
        a = list(ok); a[i] = C.c_void_p(P + 8)
        assert f(*a) == ERR_ARG, i
    for i in (1, 3, 15):                                            # strides: multiples of 8 that cover the channels
        for ld in (56, 68):
            a = list(ok); a[i] = ld
            assert f(*a) == ERR_ARG, (i, ld)
    for T, C_ in ((0, 64), (800, 0), (800, 12), (800, 1032), (1 << 31, 64)):
        a = list(ok); a[4], a[5] = T, C_
        assert f(*a) == ERR_ARG, (T, C_)


# ------------------------------------------------------------------------------------------------ route
def route_and_instance(B, H, k, cin, cout, ws_bytes=yv.CONV_WS_BYTES):
    r = yv.conv_bnbwd_route(B, H, H, k, 1, cin, cout, ws_bytes=ws_bytes)
    code = yv.lib.yv_conv2d_instance(B, H, H, k, 1, cin, 0, cout, cout, cout, yv.EPI_RES_BF16, ws_bytes)
    assert code >= 0
    return r, code


ROUTE_SHAPES = [(16, 40, 3, 64, 64), (16, 20, 3, 256, 256), (2, 20, 1, 512, 256), (16, 160, 3, 32, 32), (16, 40, 1, 80, 128),
                (2, 20, 3, 128, 128), (16, 320, 3, 32, 16)]           # none of them is one the route sends back on time (below)


def test_route_use_is_false_exactly_where_the_unfused_call_splits_k():
    """Under the shipped options nothing splits; with "conv_splitk" = 1 the deep 20 x 20 layers do, and there - and only there -
    `use` is False.  The route's own instance never has the split bit and equals yv_conv2d_instance's without a workspace."""
    old = yv.get_option("conv_splitk")
    try:
        yv.set_option("conv_splitk", 0)
        for shape in ROUTE_SHAPES:
            r, code = route_and_instance(*shape)
            assert not code & yv.CONV_SPLITK and r.use and not r.splitk, shape
            assert (r.kernel, r.staged) == (code & 15, bool(code & yv.CONV_STAGED)), shape
            B, H, _, _, cout = shape
            assert r.tiles == -(-B * H * H // 128) and r.workgroups % r.tiles == 0 and r.workgroups >= r.tiles
        yv.set_option("conv_splitk", 1)
        split = []
        for shape in ROUTE_SHAPES:
            r, code = route_and_instance(*shape)
            assert r.splitk == bool(code & yv.CONV_SPLITK) and r.use == (not code & yv.CONV_SPLITK), shape
            plain = yv.lib.yv_conv2d_instance(shape[0], shape[1], shape[1], shape[2], 1, shape[3], 0, shape[4], shape[4], shape[4],
                                              yv.EPI_RES_BF16, 0)
            assert (r.kernel, r.staged) == (plain & 15, bool(plain & yv.CONV_STAGED)), shape     # the fused launch itself never splits
            split.append(r.splitk)
            r0, _ = route_and_instance(*shape, ws_bytes=0)                                       # no workspace: nothing to split into
            assert r0.use and not r0.splitk
        assert any(split) and not all(split), split
    finally:
        yv.set_option("conv_splitk", old)
    assert yv.get_option("conv_splitk") == old


def test_route_sends_back_what_was_measured_slower():
    """`use` by instance and rows under the shipped options: 64- and 128-wide instances lose from 100,000 rows, the 32-wide one from
    400,000 rows with K >= 512, the 16-wide one never."""
    I16, I32, I64, I128, D64, D128 = (yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_128, yv.CONV_DMA_64_3,
                                      yv.CONV_DMA_128_2)
    table = [  # B, H, k, cin, cout -> instance, use
        ((16, 80, 3, 64, 64), D64, False), ((16, 79, 3, 64, 64), D64, True), ((16, 80, 1, 128, 128), D128, False),
        ((16, 80, 1, 80, 128), I128, False), ((16, 40, 1, 80, 128), I128, True), ((16, 80, 1, 8, 64), I64, False),
        ((16, 40, 1, 8, 64), I64, True), ((16, 320, 3, 64, 32), I32, False), ((16, 160, 3, 64, 32), I32, False),
        ((16, 158, 3, 64, 32), I32, True), ((16, 160, 3, 32, 32), I32, True), ((16, 160, 1, 32, 32), I32, True),
        ((16, 320, 3, 32, 16), I16, True), ((16, 160, 3, 16, 16), I16, True)]
    for shape, kernel, use in table:
        r, _ = route_and_instance(*shape)
        assert (r.kernel, r.use, r.splitk) == (kernel, use, False), (shape, r)


def test_route_rejects_what_the_call_rejects():
    for kw in (dict(Cout=12), dict(ldz=56), dict(ldz=68), dict(flags=yv.EPI_SILU), dict(ksize=5)):
        a = dict(B=2, Hout=20, Wout=20, ksize=3, stride=1, Cin=64, Cout=64)
        a.update(kw)
        with pytest.raises(yv.YvError):
            yv.conv_bnbwd_route(**a)


# ------------------------------------------------------------------------------------------------ the fused pairs
def _bn_keys(scale, nc):
    from yvhip.yolo_training import Block, train_launches
    return [e.key for e in train_launches(scale, nc) if isinstance(e, Block) and e.bn]


def _phase_blocks(scale, nc, size, batch):
    """What YoloTrainer(phase_dgrad=True)._phase_blocks holds: the stride-2 blocks whose phase route says `use`."""
    from yvhip.yolo_training import Block, train_launches
    out = set()
    for e in train_launches(scale, nc):
        if isinstance(e, Block) and e.stride == 2 and e.dgrad:
            try:
                if yv.conv_dgrad_s2_route(batch, size // e.down_in, size // e.down_in, e.k, e.cin, e.cout).use:
                    out.add(e.key)
            except yv.YvError:
                pass
    return out


@pytest.mark.parametrize("scale,nc", [("s", 80), ("n", 5)])
def test_eligible_set_at_16x640(scale, nc):
    from yvhip.yolo_training import fused_bn_bwd_pairs, fused_bn_bwd_plan
    keys = _bn_keys(scale, nc)
    assert len(keys) == 57 and len(ELIGIBLE) == 29 and set(ELIGIBLE) <= set(keys)
    pairs = fused_bn_bwd_pairs(scale, nc)
    assert sorted(pairs) == ELIGIBLE
    plan = fused_bn_bwd_plan(scale, nc, 640, 16)
    back = ROUTED_BACK[scale, nc]
    assert back < set(ELIGIBLE) and set(plan.values()) == set(ELIGIBLE) - back and all(pairs[p] == c for c, p in plan.items())
    assert sorted(fused_bn_bwd_plan(scale, nc, 160, 2).values()) == ELIGIBLE          # small maps: every pair is fused
    # phase_dgrad: exactly the producers whose consumer's data gradient is a phase launch drop out
    phase = _phase_blocks(scale, nc, 640, 16)
    assert phase
    with_phase = fused_bn_bwd_plan(scale, nc, 640, 16, frozenset(phase))
    lost = {p for p, c in pairs.items() if c in phase}
    assert lost and set(with_phase.values()) == set(ELIGIBLE) - back - lost
    assert lost <= {"model.0", "model.2.cv2"}                       # their consumers model.1 and model.3 are the stride-2 blocks


@pytest.mark.parametrize("scale,nc", [("s", 80), ("n", 5)])
def test_every_fused_producer_directly_follows_its_consumer(scale, nc):
    from yvhip.yolo_training import Block, fused_bn_bwd_pairs, train_backward_order
    order = [e for group in train_backward_order(scale, nc) for e in group if isinstance(e, Block)]
    at = {e.key: i for i, e in enumerate(order)}
    by_key = {e.key: e for e in order}
    for producer, consumer in fused_bn_bwd_pairs(scale, nc).items():
        assert at[producer] == at[consumer] + 1, (producer, consumer)
        assert by_key[consumer].src == by_key[producer].out and by_key[consumer].dgrad and by_key[producer].bn


# ------------------------------------------------------------------------------------------------ the launches
def record(**kw) -> dict:
    """One step of yolo_trainer_trace's case (YOLOv8n, nc 5, 64 x 64, batch 2, its batch) with the constructor arguments kw: that
    module's recorder and patches, plus a name for the fused pairs' partials buffer."""
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        for var in ytt.FLAGS + (FLAG, "YV_YOLO_GATHER_WGRAD"):
            mp.delenv(var, raising=False)
        ytt._patch(mp, rec)
        tr = YoloTrainer(init_yolo_train_state(ytt.SCALE, ytt.NC, seed=3), scale=ytt.SCALE, nc=ytt.NC, size=ytt.SIZE, batch=ytt.B,
                         device="cpu", **kw)
        g = torch.Generator().manual_seed(21)
        ctr, wh = torch.rand(ytt.B, ytt.GT, 2, generator=g) * (ytt.SIZE - 30) + 15, torch.rand(ytt.B, ytt.GT, 2, generator=g) * 20 + 8
        batch = dict(images=torch.randint(0, 256, (ytt.B, ytt.SIZE, ytt.SIZE, 3), generator=g,
                                          dtype=torch.uint8).as_subclass(ytt._DeviceImages),
                     gt_boxes=torch.cat([ctr - wh / 2, ctr + wh / 2], -1),
                     gt_labels=torch.randint(0, ytt.NC, (ytt.B, ytt.GT), generator=g, dtype=torch.int32),
                     gt_counts=torch.full((ytt.B,), ytt.GT, dtype=torch.int32))
        ytt._names(rec, tr, batch)
        if tr.bn_bwd_ws is not None:
            rec.walk("bn_bwd_ws", tr.bn_bwd_ws)
        rec.recording = True
        with tt._TorchOps(rec):
            tr.step(batch["images"], batch["gt_boxes"], batch["gt_labels"], batch["gt_counts"])
        rec.recording = False
        plan = dict(tr._bnbwd_of)
    return dict(json.loads(json.dumps({"allocs": rec.alloc_table(), "calls": rec.trace})), plan=plan)


@pytest.fixture(scope="module")
def fused():
    return record(fused_bn_bwd=True)


def test_flag_defaults_and_environment(monkeypatch):
    from utils import trainYolo as ty
    from yvhip.yolo_training import YoloTrainer
    assert inspect.signature(YoloTrainer.__init__).parameters["fused_bn_bwd"].default is None
    assert inspect.signature(ty.train).parameters["fused_bn_bwd"].default is None
    from yvhip.engines import _env_flag
    monkeypatch.delenv(FLAG, raising=False)
    assert _env_flag(None, FLAG) is False
    monkeypatch.setenv(FLAG, "1")
    assert _env_flag(None, FLAG) is True and _env_flag(False, FLAG) is False


def test_trace_with_the_flag_equals_the_fixture(fused):
    with open(FIXTURE, encoding="utf-8") as f:
        want = json.load(f)["fused_bn_bwd"]
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert fused["allocs"] == want["allocs"]
    for i, (g, w) in enumerate(zip(fused["calls"], want["calls"])):
        if g != w:
            pytest.fail(f"call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(fused["calls"]) == len(want["calls"])


def test_trace_without_the_flag_is_the_default_trace():
    """The flag-off trainer records the first step of yolo_trainer_trace's `default` fixture, line for line, and allocates what it
    allocates."""
    got, want = record(), ytt.load_fixture()["default"]
    first = want["calls"][:[i for i, c in enumerate(want["calls"]) if c[0] == "blob_nhwc8"][1]]
    assert got["plan"] == {} and got["allocs"] == want["allocs"]
    for i, (g, w) in enumerate(zip(got["calls"], first)):
        if g != w:
            pytest.fail(f"call {i} differs\n  recorded: {g}\n  default:  {w}")
    assert len(got["calls"]) == len(first)
    again = record(fused_bn_bwd=False)
    assert again["calls"] == got["calls"] and again["allocs"] == got["allocs"]


def test_the_fused_trace_holds_what_it_must(fused):
    """bn_act_bwd runs for the ineligible producers only, bn_act_bwd_finish once per eligible one, right behind the data gradient
    that left its sums; every other call is the default trainer's."""
    calls, plan = fused["calls"], fused["plan"]
    assert sorted(plan.values()) == ELIGIBLE                      # 64 x 64, batch 2: no route splits K
    assert "bn_bwd_ws" in fused["allocs"] and "bn_bwd_ws" not in record()["allocs"]
    key_of = lambda operand: operand.split("@")[0].split("[")[0][len("dz."):]
    plain = [key_of(c[2][9]) for c in calls if c[0] == "bn_act_bwd"]           # the dz operand names the block
    finish = [key_of(c[2][9]) for c in calls if c[0] == "bn_act_bwd_finish"]
    assert sorted(finish) == ELIGIBLE and len(set(finish)) == len(finish)
    assert sorted(plain) == sorted(set(_bn_keys(ytt.SCALE, ytt.NC)) - set(ELIGIBLE)) and len(plain) == 57 - 29
    names = [c[0] for c in calls]
    assert names.count("conv_view_bnbwd") == 29
    main = [c for c in calls if c[1] == 0 and c[0] in ("conv_view_bnbwd", "bn_act_bwd_finish", "bn_act_bwd", "conv_view", "cast_colsum")]
    for i, c in enumerate(main):
        if c[0] == "conv_view_bnbwd":
            nxt = main[i + 1]
            assert nxt[0] == "bn_act_bwd_finish", nxt
            assert c[2][8] == nxt[2][0]                              # the convolution's output view is the finaliser's da
            assert c[2][9] == nxt[2][1] and c[2][14] == nxt[2][10] == "bn_bwd_ws"      # the producer's z; the pair's partials
            assert c[3]["res"] == c[2][8]                            # the residual read stays
    # everything else equals the flag-off trace: same calls in the same order once the three fused kinds are mapped back
    off = record()["calls"]
    back = {"conv_view_bnbwd": "conv_view", "bn_act_bwd_finish": "bn_act_bwd"}
    assert [back.get(c[0], c[0]) for c in calls] == [c[0] for c in off]
    for a, b in zip(calls, off):
        if a[0] not in back:
            assert a == b


if __name__ == "__main__":
    t = record(fused_bn_bwd=True)
    text = tt.dumps({"fused_bn_bwd": {"allocs": t["allocs"], "calls": t["calls"]}})
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"wrote {FIXTURE}: {len(text)} bytes, {text.count(chr(10))} lines")
    else:
        sys.stdout.write(text)
