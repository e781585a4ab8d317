"""The stride-2 data gradient by parity phase, as far as it goes without a GPU: the tap table yvhip.dgrad_s2_taps states (the one
yv_conv2d_dgrad_s2 walks) against autograd on integer data, and the route yv_conv2d_dgrad_s2_route reports - the function the
launch path calls decides it - for both kernel families, the rejected layers and the detector's stride-2 layers."""
import pytest
import torch
import torch.nn.functional as F

import yvhip as yv
from yvhip.yolo_training import yolo_s2_dgrad_shapes

ERR_ARG = -1
PHASES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def flipped_weight(w: torch.Tensor) -> torch.Tensor:
    """conv_weight_dgrad on the host: w (Cout, Cin, 3, 3) -> wd (Cin, 9, Cout), slot = 8 - (3 * ky + kx)."""
    cout, cin = w.shape[:2]
    return w.permute(1, 2, 3, 0).reshape(cin, 9, cout).flip(1)


def phase_dgrad(dz: torch.Tensor, wd: torch.Tensor) -> torch.Tensor:
    """dz (B, Hout, Wout, Cout), wd (Cin, 9, Cout) -> dx (B, 2 Hout, 2 Wout, Cin) by the table of dgrad_s2_taps."""
    B, Ho, Wo, _ = dz.shape
    dx = torch.zeros(B, 2 * Ho, 2 * Wo, wd.shape[0], dtype=dz.dtype)
    pad = F.pad(dz, (0, 0, 0, 1, 0, 1))                       # one zero row and column past the end
    for py, px in PHASES:
        for slot, dy, dxx in yv.dgrad_s2_taps(py, px):
            dx[:, py::2, px::2] += pad[:, dy:dy + Ho, dxx:dxx + Wo] @ wd[:, slot].T
    return dx


@pytest.mark.parametrize("B,Hin,Win,Cin,Cout", [(2, 16, 16, 32, 64), (3, 10, 10, 64, 128), (2, 12, 20, 64, 64)])
def test_tap_table_equals_autograd_on_integers(B, Hin, Win, Cin, Cout):
    g = torch.Generator().manual_seed(Hin * 1000 + Cin)
    x = torch.zeros(B, Cin, Hin, Win, dtype=torch.float64, requires_grad=True)
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).double()
    dz = torch.randint(-1, 2, (B, Cout, Hin // 2, Win // 2), generator=g).double()
    F.conv2d(x, w, stride=2, padding=1).backward(dz)
    got = phase_dgrad(dz.permute(0, 2, 3, 1).contiguous(), flipped_weight(w))
    assert torch.equal(got, x.grad.permute(0, 2, 3, 1))


def test_tap_counts_and_order():
    assert [len(yv.dgrad_s2_taps(py, px)) for py, px in PHASES] == [1, 2, 2, 4]
    seen = []
    for py, px in PHASES:
        taps = yv.dgrad_s2_taps(py, px)
        slots = [t[0] for t in taps]
        assert slots == sorted(slots)
        assert all(dy == (s // 3 == 2) and dx == (s % 3 == 2) for s, dy, dx in taps)
        seen += slots
    assert sorted(seen) == list(range(9))                     # every tap of the 3 x 3 belongs to exactly one phase


def test_route_reports_both_kernel_families():
    r = yv.conv_dgrad_s2_route(2, 16, 16, 3, 32, 64)
    assert r.kernel == yv.CONV_IGEMM_32 and not r.staged and r.ksteps == (4, 2, 2, 1)
    assert (r.tiles, r.workgroups) == (1, 4)
    r = yv.conv_dgrad_s2_route(2, 16, 16, 3, 64, 64)
    assert r.kernel == yv.CONV_DMA_64_3 and r.staged and r.ksteps == (4, 2, 2, 1)
    r = yv.conv_dgrad_s2_route(3, 10, 10, 3, 256, 128)
    assert r.kernel == yv.CONV_DMA_64_3 and r.staged and r.ksteps == (8, 4, 4, 2)
    assert (r.tiles, r.workgroups) == (4, 16)                  # 75 rows: one row tile, four 64-column tiles, four phases
    assert yv.conv_dgrad_s2_route(16, 320, 320, 3, 128, 64).kernel == yv.CONV_DMA_128_2        # >= 100 k rows, N > 64
    assert yv.conv_dgrad_s2_route(2, 16, 16, 3, 48, 64).kernel == yv.CONV_IGEMM_64
    assert yv.conv_dgrad_s2_route(2, 16, 16, 3, 16, 64).kernel == yv.CONV_IGEMM_16


@pytest.mark.parametrize("args", [
    dict(Cout=32), dict(ksize=1), dict(Hin=15), dict(Win=15), dict(Cin=4), dict(Cout=96), dict(dx_ld=36), dict(dz_ld=60), dict(B=0)])
def test_route_rejects_what_the_entry_rejects(args):
    a = dict(B=2, Hin=16, Win=16, ksize=3, Cin=32, Cout=64, dz_ld=None, dx_ld=None)
    a.update(args)
    out = (yv.C.c_int * 9)()
    dz_ld = a["Cout"] if a["dz_ld"] is None else a["dz_ld"]
    dx_ld = a["Cin"] if a["dx_ld"] is None else a["dx_ld"]
    assert yv.lib.yv_conv2d_dgrad_s2_route(a["B"], a["Hin"], a["Win"], a["ksize"], a["Cin"], a["Cout"], dz_ld, dx_ld, dx_ld,
                                           out) == ERR_ARG
    with pytest.raises(yv.YvError):
        yv.conv_dgrad_s2_route(a["B"], a["Hin"], a["Win"], a["ksize"], a["Cin"], a["Cout"], a["dz_ld"], a["dx_ld"])


def eligible(scale):
    out = {}
    for key, hin, cin, cout in yolo_s2_dgrad_shapes(scale, 640):
        try:
            yv.conv_dgrad_s2_route(16, hin, hin, 3, cin, cout)
            out[key] = True
        except yv.YvError:
            out[key] = False
    return out


def test_detector_layers():
    keys = ["model.1", "model.3", "model.5", "model.7", "model.16", "model.19"]
    assert [k for k, *_ in yolo_s2_dgrad_shapes("s")] == keys
    assert eligible("s") == {k: True for k in keys}
    assert eligible("n") == {k: k != "model.1" for k in keys}          # YOLOv8n's model.1 has 32 output channels
    # model.1 of YOLOv8s: 32 gradient columns over 1.6 M rows, the igemm form
    key, hin, cin, cout = yolo_s2_dgrad_shapes("s")[0]
    r = yv.conv_dgrad_s2_route(16, hin, hin, 3, cin, cout)
    assert (cin, cout, r.kernel) == (32, 64, yv.CONV_IGEMM_32) and r.tiles == 16 * 160 * 160 // 128
    key, hin, cin, cout = yolo_s2_dgrad_shapes("n")[1]                  # model.3 of YOLOv8n: the same width
    assert (key, cin, cout) == ("model.3", 32, 64) and yv.conv_dgrad_s2_route(16, hin, hin, 3, cin, cout).kernel == yv.CONV_IGEMM_32
