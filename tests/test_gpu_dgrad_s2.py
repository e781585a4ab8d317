"""The stride-2 data gradient by parity phase (yv_conv2d_dgrad_s2) on the GPU: exact integers against autograd and against the
zero-insert path for both kernel families, ragged tiles, H != W, several row / column tiles and channel slices of wider buffers;
normal-distributed data against the zero-insert path bit for bit; the rejected arguments; and YoloTrainer(phase_dgrad=True)
through the trainer's own checks.

Integer operands ({-1, 0, 1} weights and gradients, a [-8, 8] residual): every product and every f32 partial sum is an exact
integer, and the cases assert |grad| <= 256 and |prev + grad| <= 256 before they launch, so every value is a bf16 number under
either rounding form of the epilogue.  A wrong tap, displacement, wd column, validity bit or output row is then a wrong integer
somewhere, and the comparisons are torch.equal.  The gradient has loud first / last rows and columns in every image (+1 / -1 in
every channel of the buffer, read or not): a + 1 tap that reads the next row, or the next image, instead of zero changes a sum.

Established on the MI355X (test_normal_data_has_the_bits_of_the_zero_insert_path): where the two paths take the same epilogue
form and neither splits K, they give the same bits - the zero-insert convolution's other K steps add products with zeros."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0.5
ERR_ARG = -1


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def bf(t):
    return t.to(torch.bfloat16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def operands(B, Hin, Win, Cin, Cout, integer):
    """CPU operands of a case and the float64 autograd gradient, NHWC: (w (Cout,3,3,Cin), dz (B,Hout,Wout,Cout), prev, grad)."""
    g = torch.Generator().manual_seed(B * 7 + Hin * 1000 + Win * 10 + Cin + Cout)
    Hout, Wout = Hin // 2, Win // 2
    if integer:
        w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).double()
        dz = torch.randint(-1, 2, (B, Cout, Hout, Wout), generator=g).double()
        dz[:, :, 0] = 1; dz[:, :, :, 0] = 1; dz[:, :, -1] = -1; dz[:, :, :, -1] = -1
        prev = torch.randint(-8, 9, (B, Hin, Win, Cin), generator=g).double()
    else:
        w = bf(torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cout) ** -0.5).double()
        dz = bf(torch.randn(B, Cout, Hout, Wout, generator=g)).double()
        prev = bf(torch.randn(B, Hin, Win, Cin, generator=g)).double()
    x = torch.zeros(B, Cin, Hin, Win, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, stride=2, padding=1).backward(dz)
    return w.permute(0, 2, 3, 1).contiguous(), dz.permute(0, 2, 3, 1).contiguous(), prev, x.grad.permute(0, 2, 3, 1).contiguous()


def device_buffers(yv, B, Hin, Win, Cin, Cout, integer, dz_off=0, dz_pad=0, dx_off=0, dx_pad=0):
    """dz and dx as channel slices [off, off + C) of buffers `pad` channels wider; the rest of dz is loud, the rest of dx the sentinel."""
    w, dz, prev, grad = operands(B, Hin, Win, Cin, Cout, integer)
    Hout, Wout = Hin // 2, Win // 2
    wk = bf(w.reshape(Cout, 9 * Cin)).to(DEV)
    wd = torch.empty(Cin, 9 * Cout, dtype=torch.bfloat16, device=DEV)
    yv.conv_weight_dgrad(wk, Cout, 9, Cin, wd)
    dzb = torch.full((B, Hout, Wout, Cout + dz_pad), 1.0, dtype=torch.bfloat16, device=DEV)
    dzb[..., dz_off:dz_off + Cout] = bf(dz).to(DEV)
    dxb = torch.full((B, Hin, Win, Cin + dx_pad), SENTINEL, dtype=torch.bfloat16, device=DEV)
    dxb[..., dx_off:dx_off + Cin] = bf(prev).to(DEV)
    return wd, dzb, dxb, prev, grad


def run_phase(yv, B, Hin, Win, Cin, Cout, wd, dzb, dxb, dz_off=0, dx_off=0):
    out = dxb.clone()
    yv.conv_dgrad_s2(yv.mview(dzb, dz_off, Cout), B, Hin // 2, Win // 2, wd, Cin, Cout, yv.mview(out, dx_off, Cin),
                     res=yv.mview(out, dx_off, Cin))
    return out


def run_zero_insert(yv, B, Hin, Win, Cin, Cout, wd, dzb, dxb, dz_off=0, dx_off=0):
    """What YoloTrainer._bwd launches without the flag: zero insertion, then a stride-1 convolution with the same wd."""
    out = dxb.clone()
    zi = torch.full((B, Hin, Win, Cout), 3.0, dtype=torch.bfloat16, device=DEV)
    yv.view_op(yv.VIEW_ZERO_INSERT, yv.mview(dzb, dz_off, Cout), yv.mview(zi), B, Hin // 2, Win // 2)
    yv.conv_view(yv.mview(zi), B, Hin, Win, 3, 1, wd.view(Cin, 9 * Cout), Cin, yv.mview(out, dx_off, Cin), res=yv.mview(out, dx_off, Cin))
    return out


INTEGER_CASES = [
    # B, Hin, Win, Cin, Cout, route, slices (dz_off, dz_pad, dx_off, dx_pad)
    pytest.param(2, 16, 16, 32, 64, "CONV_IGEMM_32", (0, 0, 0, 0), id="igemm-form"),
    pytest.param(2, 16, 16, 64, 64, "CONV_DMA_64_3", (0, 0, 0, 0), id="dma-form-one-tile"),
    pytest.param(3, 10, 10, 64, 128, "CONV_DMA_64_3", (0, 0, 0, 0), id="ragged-last-tile-75-rows"),
    pytest.param(2, 12, 20, 64, 64, "CONV_DMA_64_3", (0, 0, 0, 0), id="h-not-w"),
    pytest.param(2, 24, 24, 64, 64, "CONV_DMA_64_3", (0, 0, 0, 0), id="three-row-tiles"),
    pytest.param(1, 8, 8, 256, 64, "CONV_DMA_64_3", (0, 0, 0, 0), id="two-column-tiles"),
    pytest.param(2, 16, 16, 64, 128, "CONV_DMA_64_3", (8, 16, 16, 24), id="channel-slices-of-wider-buffers"),
]


@pytest.mark.parametrize("B,Hin,Win,Cin,Cout,route,sl", INTEGER_CASES)
def test_exact_integers(yv, B, Hin, Win, Cin, Cout, route, sl):
    dz_off, dz_pad, dx_off, dx_pad = sl
    r = yv.conv_dgrad_s2_route(B, Hin, Win, 3, Cin, Cout, Cout + dz_pad, Cin + dx_pad)
    assert r.kernel == getattr(yv, route) and r.staged == (r.kernel >= yv.CONV_IGEMM_64)
    wd, dzb, dxb, prev, grad = device_buffers(yv, B, Hin, Win, Cin, Cout, True, dz_off, dz_pad, dx_off, dx_pad)
    assert float(grad.abs().max()) <= 256 and float((prev + grad).abs().max()) <= 256     # exact in bf16, either rounding form
    exp = dxb.clone().cpu()
    exp[..., dx_off:dx_off + Cin] = bf(prev + grad)
    got = run_phase(yv, B, Hin, Win, Cin, Cout, wd, dzb, dxb, dz_off, dx_off)
    ref = run_zero_insert(yv, B, Hin, Win, Cin, Cout, wd, dzb, dxb, dz_off, dx_off)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), exp)                        # prev + autograd in the slice, the sentinel everywhere else
    assert torch.equal(got, ref)                              # and the zero-insert path on the same buffers


@pytest.mark.parametrize("B,Hin,Win,Cin,Cout", [(2, 16, 16, 32, 64), (2, 24, 24, 128, 256)])
def test_normal_data_has_the_bits_of_the_zero_insert_path(yv, B, Hin, Win, Cin, Cout):
    """Same products, same f32 accumulation order over the non-zero K steps, same epilogue form (asserted): the same bits.  Both
    errors against the float64 gradient are printed."""
    r = yv.conv_dgrad_s2_route(B, Hin, Win, 3, Cin, Cout)
    code = yv.conv2d_instance(B, Hin, Win, 3, 1, Cout, 0, Cin, Cin, Cin, yv.EPI_RES_BF16)
    assert not code & yv.CONV_SPLITK and bool(code & yv.CONV_STAGED) == r.staged
    wd, dzb, dxb, prev, grad = device_buffers(yv, B, Hin, Win, Cin, Cout, False)
    got = run_phase(yv, B, Hin, Win, Cin, Cout, wd, dzb, dxb)
    ref = run_zero_insert(yv, B, Hin, Win, Cin, Cout, wd, dzb, dxb)
    torch.cuda.synchronize()
    e_phase, e_zi = rel_l2(got.cpu(), prev + grad), rel_l2(ref.cpu(), prev + grad)
    print(f"rel_l2 against float64: phase {e_phase:.3e}, zero-insert {e_zi:.3e}, "
          f"elements that differ {int((got != ref).sum())} of {got.numel()}")
    assert e_zi < 8e-3                                        # (the reference path itself: two bf16 roundings at most)
    assert torch.equal(got, ref)


def test_ineligible_arguments_leave_dx_untouched(yv):
    B, Hout, Cin, Cout = 2, 8, 32, 64
    wd = torch.ones(Cin * 9 * Cout + 8, dtype=torch.bfloat16, device=DEV)
    dz = torch.ones(B, Hout, Hout, Cout + 8, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((B, 2 * Hout, 2 * Hout, Cin + 8), SENTINEL, dtype=torch.bfloat16, device=DEV)
    C = yv.C

    def call(dz_off=0, dz_c=Cout, dz_ld=Cout + 8, up=0, b=B, cin=Cin, cout=Cout, dx_off=0, dx_ld=Cin + 8, res_off=0, res_ld=Cin + 8,
             wd_off=0, null=None):
        v = yv.yv_view(C.c_void_p(dz.data_ptr() + 2 * dz_off), dz_ld, dz_c, up)
        ptr = {"wd": wd.data_ptr() + 2 * wd_off, "dx": dx.data_ptr() + 2 * dx_off, "res": dx.data_ptr() + 2 * res_off}
        ptr = {k: None if k == null else C.c_void_p(p) for k, p in ptr.items()}
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return yv.lib.yv_conv2d_dgrad_s2(C.byref(v) if null != "dz" else None, b, Hout, Hout, ptr["wd"], cin, cout, ptr["dx"], dx_ld,
                                         ptr["res"], res_ld, None, 0, stream)

    bad = [dict(cout=32, dz_c=32), dict(cout=96, dz_c=96), dict(cin=4), dict(cin=36), dict(dz_c=32), dict(up=1), dict(b=0),
           dict(dz_off=4), dict(dx_off=4), dict(res_off=4), dict(wd_off=4), dict(dz_ld=Cout + 4), dict(dx_ld=Cin + 4),
           dict(res_ld=Cin + 4), dict(dx_ld=Cin - 8), dict(dz_ld=Cout - 8), dict(null="dz"), dict(null="wd"), dict(null="dx")]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all())
    assert call() == 0 and call(null="res") == 0               # the same arguments, eligible: accepted
    torch.cuda.synchronize()
    assert bool((dx[..., :Cin] != SENTINEL).all()) and bool((dx[..., Cin:] == SENTINEL).all())


def test_trainer_phase_dgrad_passes_the_trainer_checks(yv, monkeypatch):
    """YV_YOLO_PHASE_DGRAD=1: the project's own trainer checks (tests/test_gpu_yolo_train.py, their tolerances: outputs 6e-3,
    gradients 3e-2, the loss comes down) pass; per backward pass (1 + 12 training steps) zero insertion runs once, for
    YOLOv8n's model.1 (32 output channels: not eligible), and conv_dgrad_s2 five times (model.3, 5, 7, 16, 19).  Then, from one
    state and one batch, the flag changes no bit of any parameter gradient (see the test above)."""
    import yvhip.yolo_training as yt
    from test_gpu_yolo_train import test_trainer_local_consistency, test_training_steps_reduce_the_loss
    monkeypatch.setenv("YV_YOLO_PHASE_DGRAD", "1")
    probe = yt.YoloTrainer(yt.init_yolo_train_state("n", 5, seed=1), scale="n", nc=5, size=160, batch=2)
    assert probe.phase_dgrad is True
    assert sorted(probe._phase_blocks) == sorted(["model.3", "model.5", "model.7", "model.16", "model.19"])
    del probe
    zero_inserts, phase_calls = [], [0]
    real_view_op, real_dgrad = yt.view_op, yt.conv_dgrad_s2

    def view_op(mode, src, dst, B, H, W, *a, **kw):
        if mode == yv.VIEW_ZERO_INSERT:
            zero_inserts.append((src.c, H))
        return real_view_op(mode, src, dst, B, H, W, *a, **kw)

    def conv_dgrad_s2(*a, **kw):
        phase_calls[0] += 1
        return real_dgrad(*a, **kw)

    monkeypatch.setattr(yt, "view_op", view_op)
    monkeypatch.setattr(yt, "conv_dgrad_s2", conv_dgrad_s2)
    test_trainer_local_consistency(yv, "n", 5, 160, 2)
    test_training_steps_reduce_the_loss(yv)
    assert zero_inserts == [(32, 40)] * 13, zero_inserts       # model.1 at 160 x 160: dz (B, 40, 40, 32)
    assert phase_calls[0] == 5 * 13
    monkeypatch.undo()

    sd = yt.init_yolo_train_state("n", 5, seed=1)
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 160, 160, 3), generator=g, dtype=torch.uint8).to(DEV)
    grads = []
    for flag in (False, True):
        tr = yt.YoloTrainer({k: v.clone() for k, v in sd.items()}, scale="n", nc=5, size=160, batch=2, phase_dgrad=flag)
        assert len(tr._phase_blocks) == (5 if flag else 0)
        outs = tr.forward(img)
        gr = torch.Generator().manual_seed(12)
        R = [(bf(torch.randn(o[0].shape, generator=gr)).float().to(DEV), bf(torch.randn(o[1].shape, generator=gr)).float().to(DEV))
             for o in outs]
        tr.backward(R)
        torch.cuda.synchronize()
        grads.append(tr.G.cpu().clone())
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1])
