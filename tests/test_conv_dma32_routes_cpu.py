"""The 32-aligned step of conv_route ("conv_dma32", "conv_dma32_cols"; cgemm_dma32_kernel<64, ..> = CONV_DMA32_64 and
<128, ..> = CONV_DMA32_128; the 96-wide instance, code 12, measured fastest on no layer and is not built) as
yv_conv2d_instance reports it, without a GPU: off by default and then igemm_kernel's codes, as on the parent
commit; with the option on, the eligibility edges, the forced instances, the staged bit of each, the trainer-side queries and
the grouped partition untouched, and the layers of each detector scale that take a new code (engines.dma32_layers).

The convolution has no device row count (m_dev is an argument of the linears only), so that clause of the eligibility has no
query that reaches it."""
import contextlib

import pytest

import yvhip as yv
from yvhip import engines

SHIPPED = {"conv_dma": 8, "conv_splitk": 0, "staged_epilogue": 1, "conv_small": 0, "conv_small_rows": 0, "conv_dma32": 0,
           "conv_dma32_cols": 0}
ST, SK, TWO = yv.CONV_STAGED, yv.CONV_SPLITK, yv.CONV_TWO
I64, I128, D64 = yv.CONV_IGEMM_64 | ST, yv.CONV_IGEMM_128 | ST, yv.CONV_DMA_64_3 | ST
NEW = {64: yv.CONV_DMA32_64 | ST, 128: yv.CONV_DMA32_128 | ST}      # both run the staged epilogue
ANY = tuple(NEW.values())
COLS = tuple(NEW)


@contextlib.contextmanager
def options(**kw):
    want = dict(SHIPPED, **kw)
    old = {k: yv.get_option(k) for k in want}
    try:
        for k, v in want.items():
            yv.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def inst(B, H, W, k, s, c0, c1, cout, out_ld=None, **kw):
    return yv.conv2d_instance(B, H, W, k, s, c0, c1, cout, cout if out_ld is None else out_ld, **kw)


# (shape, the parent commit's code): the shapes of tests/test_gpu_conv_dma32.py and the engine's layer classes
OFF = [((1, 5, 7, 3, 1, 96, 0, 64), I64), ((2, 5, 7, 3, 1, 96, 0, 96), I128), ((1, 5, 7, 1, 1, 32, 0, 64), I64),
       ((2, 5, 7, 1, 1, 96, 0, 72), I128), ((1, 9, 9, 1, 1, 160, 0, 128), I128), ((1, 9, 9, 3, 1, 288, 0, 288), I128),
       ((2, 9, 9, 3, 2, 96, 0, 192), I128), ((1, 5, 7, 3, 2, 32, 0, 64), I64), ((1, 8, 10, 1, 1, 96, 32, 64), I64 | TWO),
       ((1, 8, 10, 1, 1, 32, 96, 128), I128 | TWO), ((64, 80, 80, 3, 1, 96, 0, 96), I128), ((64, 20, 20, 3, 1, 288, 0, 288), I128),
       ((64, 80, 80, 3, 2, 96, 0, 192), I128), ((32, 160, 160, 3, 2, 32, 0, 64), I64),
       # and what the step never takes: 64-aligned, narrow, unaligned
       ((2, 20, 20, 3, 1, 64, 0, 64), D64), ((2, 20, 20, 3, 1, 128, 0, 128), D64), ((2, 20, 20, 3, 1, 96, 0, 56), I64),
       ((2, 12, 12, 3, 1, 24, 0, 16), yv.CONV_IGEMM_16), ((2, 20, 20, 3, 1, 48, 0, 64), I64)]


def test_codes():
    assert (yv.CONV_DMA32_64, yv.CONV_DMA32_96, yv.CONV_DMA32_128) == (11, 12, 13)
    old = [yv.CONV_IGEMM_16, yv.CONV_IGEMM_32, yv.CONV_IGEMM_64, yv.CONV_IGEMM_128, yv.CONV_DMA_64_2, yv.CONV_DMA_64_3,
           yv.CONV_DMA_64_4, yv.CONV_DMA_128_2, yv.CONV_DMA_128_3, yv.CONV_SMALL_64, yv.CONV_SMALL_32]
    assert len(set(old + [11, 12, 13])) == 14 and yv.CONV_DMA32_128 < ST


def test_off_by_default_and_then_the_parent_routes():
    assert yv.get_option("conv_dma32") == 0 and yv.get_option("conv_dma32_cols") == 0
    for shape, code in OFF:
        assert inst(*shape) == code, shape
    for cols in (64, 96, 128):                       # the force option alone switches nothing on (96: no such instance)
        with options(conv_dma32_cols=cols):
            for shape, code in OFF:
                assert inst(*shape) == code, (cols, shape)
    for sc in "nsm":
        assert engines.dma32_layers(sc, 80, 4, (640, 640)) == []


def test_options_reach_set_get_and_the_environment():
    import os
    import subprocess
    import sys
    with options(conv_dma32=1, conv_dma32_cols=64):
        assert (yv.get_option("conv_dma32"), yv.get_option("conv_dma32_cols")) == (1, 64)
    code = ("import sys; sys.path.insert(0, %r); import yvhip; "
            "print(yvhip.get_option('conv_dma32'), yvhip.get_option('conv_dma32_cols'))" % os.path.dirname(os.path.dirname(yv.__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, YV_OPTIONS="conv_dma32=1,conv_dma32_cols=128"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[-2:] == ["1", "128"], r.stderr[-500:]


@pytest.mark.parametrize("cols", COLS)
def test_forced_instances_and_their_staged_bit(cols):
    with options(conv_dma32=1, conv_dma32_cols=cols):
        for shape, off in OFF[:14]:
            assert inst(*shape) == NEW[cols], shape             # staged; no split, no two-source bit
        for shape, off in OFF[14:]:
            assert inst(*shape) == off, shape


def test_no_route_reports_the_unbuilt_96_wide_instance():
    """"conv_dma32_cols" = 96 is no instance: the measured rule answers."""
    with options(conv_dma32=1):
        rule = [inst(*shape) for shape, _ in OFF]
    with options(conv_dma32=1, conv_dma32_cols=96):
        assert [inst(*shape) for shape, _ in OFF] == rule
    assert all(c & 15 != yv.CONV_DMA32_96 for c in rule)


def test_measured_rule():
    """profiles/conv_dma32_layers.txt: 128-wide tiles from 25,600 output pixels on K < 1024, 64-wide tiles otherwise, Cout = 64 on
    igemm_kernel as before."""
    with options(conv_dma32=1):
        assert inst(64, 80, 80, 3, 1, 96, 0, 96) == NEW[128] and inst(4, 80, 80, 3, 1, 96, 0, 96) == NEW[128]     # M = 25,600
        assert inst(4, 80, 79, 3, 1, 96, 0, 96) == NEW[64] and inst(1, 80, 80, 3, 1, 96, 0, 96) == NEW[64]
        assert inst(64, 160, 160, 1, 1, 96, 0, 96) == NEW[128] and inst(64, 80, 80, 3, 2, 96, 0, 192) == NEW[128]
        assert inst(64, 20, 20, 3, 1, 288, 0, 288) == NEW[64] and inst(1, 20, 20, 3, 1, 288, 0, 288) == NEW[64]   # K = 2,592
        assert inst(64, 80, 80, 1, 1, 1056, 0, 96) == NEW[64]                                                      # K >= 1024
        for shape in ((32, 160, 160, 3, 2, 32, 0, 64), (32, 80, 80, 3, 2, 32, 0, 64), (32, 80, 80, 1, 1, 96, 0, 64),
                      (1, 20, 20, 3, 1, 96, 0, 64)):
            assert inst(*shape) == I64, shape
        assert inst(1, 20, 20, 3, 1, 96, 0, 72) == NEW[64]


def test_eligibility_edges():
    with options(conv_dma32=1, conv_dma32_cols=64):
        # input channels: 32 and 96 yes, 64 and 128 keep cgemm_dma_kernel, 48 keeps igemm_kernel
        assert inst(2, 20, 20, 3, 1, 32, 0, 64) in ANY and inst(2, 20, 20, 3, 1, 96, 0, 64) in ANY
        assert inst(2, 20, 20, 3, 1, 64, 0, 64) == D64 and inst(2, 20, 20, 3, 1, 128, 0, 64) == D64
        assert inst(2, 20, 20, 3, 1, 48, 0, 64) == I64 and inst(2, 20, 20, 3, 1, 80, 0, 64) == I64
        # output channels: from 64
        assert inst(2, 20, 20, 3, 1, 96, 0, 56) == I64 and inst(2, 20, 20, 3, 1, 96, 0, 64) in ANY
        # two sources: a 1 x 1 whose first source ends on a 32-channel boundary
        assert inst(2, 20, 20, 1, 1, 96, 32, 64) in ANY and inst(2, 20, 20, 1, 1, 32, 64, 64) in ANY
        assert inst(2, 20, 20, 1, 1, 48, 48, 64) == I64 | TWO                          # c0 = 48
        assert inst(2, 20, 20, 1, 1, 64, 64, 64) == D64                                # 64-aligned: its own route
        assert yv.lib.yv_conv2d_instance(2, 20, 20, 3, 1, 64, 32, 64, 64, 0, yv.EPI_BIAS, 0) == -1      # a two-source 3 x 3
        # an output or shortcut that cannot be staged
        assert inst(2, 20, 20, 3, 1, 96, 0, 64, out_ld=68) == yv.CONV_IGEMM_64
        assert inst(2, 20, 20, 3, 1, 96, 0, 64, res_ld=68, flags=yv.EPI_RES_BF16) == yv.CONV_IGEMM_64
        assert inst(2, 20, 20, 3, 1, 96, 0, 64, res_ld=72, flags=yv.EPI_RES_BF16) in ANY
        assert inst(2, 20, 20, 3, 1, 96, 0, 64, flags=yv.EPI_OUT_F32 | yv.EPI_SILU) in ANY
    with options(conv_dma32=1, conv_dma32_cols=64, staged_epilogue=0):
        assert inst(2, 20, 20, 3, 1, 96, 0, 64) == yv.CONV_IGEMM_64
    with options(conv_dma32=1, conv_dma32_cols=64, conv_dma=0):                                            # not tied to "conv_dma"
        assert inst(2, 20, 20, 3, 1, 96, 0, 64) in ANY and inst(2, 20, 20, 3, 1, 64, 0, 64) == I64


def test_behind_splitk():
    shape = (2, 20, 20, 3, 1, 96, 0, 96)                                               # M = 800: what split-K takes with a workspace
    with options(conv_splitk=1):
        off = inst(*shape)
        assert off == yv.CONV_IGEMM_128 | SK
    with options(conv_splitk=1, conv_dma32=1, conv_dma32_cols=128):
        assert inst(*shape) == off                                                     # the split launch keeps igemm_kernel
        assert inst(*shape, ws_bytes=0) == NEW[128]                                    # yv_conv2d: no workspace, no split


def test_composes_with_small_maps():
    """Disjoint eligibility: each option takes its own layers whatever the other says."""
    with options(conv_dma32=1, conv_dma32_cols=64, conv_small=1 << 20, conv_small_fill=1 << 20):
        assert inst(1, 20, 20, 3, 1, 96, 0, 96) == NEW[64]
        assert inst(1, 20, 20, 3, 1, 128, 0, 128) in (yv.CONV_SMALL_64, yv.CONV_SMALL_32)


def test_training_routes_do_not_see_the_option():
    def training():
        rs = [yv.conv_bnbwd_route(2, 20, 20, 3, 1, 96, 96), yv.conv_bnbwd_route(1, 20, 20, 1, 1, 288, 96),
              yv.conv_bnbwd_route(64, 80, 80, 3, 1, 96, 96), yv.conv_dgrad_s2_route(2, 40, 40, 3, 96, 192),
              yv.conv_dgrad_s2_route(2, 40, 40, 3, 32, 64)]
        return [tuple(getattr(r, f) for f in r._fields) if hasattr(r, "_fields") else repr(r) for r in rs]

    with options():
        off = training()
    for cols in (0,) + COLS:
        with options(conv_dma32=1, conv_dma32_cols=cols):
            assert training() == off, cols


def test_group_plan_leaves_a_dma32_member_alone():
    """conv_group_partition groups instances 5, 9 and 10 only: a member on a new code is a launch of its own."""
    shapes = [(1, 20, 20, 3, 1, 128, 0, 128, 128), (1, 20, 20, 3, 1, 96, 0, 96, 96), (1, 10, 10, 3, 1, 128, 0, 128, 128),
              (1, 10, 10, 3, 1, 288, 0, 288, 288)]
    with options():
        n_off, off = yv.conv2d_group_plan(shapes)
    assert [m["instance"] for m in off] == [D64, I128, D64, I128] and n_off == 3
    for cols in COLS:
        with options(conv_dma32=1, conv_dma32_cols=cols):
            n_on, on = yv.conv2d_group_plan(shapes)
        assert n_on == n_off
        assert [m["instance"] for m in on] == [D64, NEW[cols], D64, NEW[cols]]
        for a, b in zip(on, off):
            assert {k: v for k, v in a.items() if k != "instance"} == {k: v for k, v in b.items() if k != "instance"}
        assert on[0]["launch"] == on[2]["launch"] and len({on[0]["launch"], on[1]["launch"], on[3]["launch"]}) == 3
    assert all(c & 15 not in yv.CONV_GROUP_INSTANCES for c in ANY)


M22 = (["model.2.cv1.conv", "model.3.conv"] + [f"model.4.m.{j}.cv{i}.conv" for j in range(4) for i in (1, 2)] +
       [f"model.8.m.{j}.cv{i}.conv" for j in range(2) for i in (1, 2)] + [f"model.15.m.{j}.cv{i}.conv" for j in range(2) for i in (1, 2)] +
       [f"model.21.m.{j}.cv{i}.conv" for j in range(2) for i in (1, 2)])


@pytest.mark.parametrize("cols", (0,) + COLS)
def test_dma32_layers_of_each_scale(cols):
    """YOLOv8m: the 96 -> 96 cv1 of model.2, model.3 (96 -> 192, stride 2) and the twenty 96- and 288-channel bottleneck
    convolutions.  YOLOv8s: model.1 (32 -> 64, stride 2).  YOLOv8n: model.3 (32 -> 64, stride 2) and the cv2 of model.15, a 1 x 1
    from the block's 3 x 32 = 96 concatenated channels to 64 - under the force option; the measured rule (cols = 0) leaves
    Cout = 64, i.e. all three, on igemm_kernel."""
    with options(conv_dma32=1, conv_dma32_cols=cols):
        for B in (4, 64):
            assert engines.dma32_layers("m", 80, B, (640, 640)) == M22 and len(M22) == 22
        assert engines.dma32_layers("s", 80, 32, (640, 640)) == (["model.1.conv"] if cols else [])
        assert engines.dma32_layers("n", 80, 32, (640, 640)) == (["model.3.conv", "model.15.cv2.conv"] if cols else [])
        assert engines.dma32_layers("m", 5, 64, (384, 640)) == M22


