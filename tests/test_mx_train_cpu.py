"""CPU checks of the MXFP8 fine-tune recipe (VitTrainer(dtype="mxfp8")): host-side argument rejection of its entry points
(no GPU call is made: every case fails validation first), the trainer's recipe / shape rule, the emulation's recipe, and
that the synthetic task of the GPU convergence test is learnable by the fp32 oracle within the GPU test's step budget."""
import ctypes as C
import types

import pytest
import torch

import yvhip

ERR_ARG = -1
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced


def _q2d(ldx=128, T=100, Cc=128, q=P, ldq=128, s=P, rows_pad=128, qt=P, ldqt=128, st=P, c_rows_pad=128, T_pad=128):
    return yvhip.lib.yv_quant_mxfp8_2d(P, ldx, T, Cc, q, ldq, s, rows_pad, qt, ldqt, st, c_rows_pad, T_pad, None)


def test_quant_mxfp8_2d_rejects_bad_arguments():
    assert _q2d(Cc=96, ldx=96) == ERR_ARG                        # C not a multiple of 128
    assert _q2d(ldx=130) == ERR_ARG                              # misaligned row stride of x
    assert _q2d(ldq=120) == ERR_ARG                              # row-form stride below C / not 16-byte aligned
    assert _q2d(rows_pad=64) == ERR_ARG                          # row-form scale rows below T
    assert _q2d(T_pad=100) == ERR_ARG                            # T_pad not a multiple of 128
    assert _q2d(T=200, rows_pad=256, T_pad=128, ldqt=256) == ERR_ARG  # T_pad below T
    assert _q2d(ldqt=136, T_pad=128) == ERR_ARG                  # column-form stride not 16-byte aligned
    assert _q2d(c_rows_pad=64) == ERR_ARG                        # column-form scale rows below C
    assert _q2d(q=None, qt=None) == ERR_ARG                      # no form requested
    assert _q2d(q=None) == ERR_ARG                               # bytes and scales of a form go together
    assert yvhip.lib.yv_quant_mxfp8_2d(P + 8, 128, 100, 128, P, 128, P, 128, None, 0, None, 0, 0, None) == ERR_ARG


def _lin(lda=256, M=256, N=256, K=256, ldo=256, flags=0, res=None, aux=None, ldaux=0, a_rows=256, w_rows=256, bias=None):
    return yvhip.lib.yv_linear_mxfp8_ex(P, lda, P, a_rows, P, P, w_rows, bias, M, N, K, P, ldo, flags, res, aux, ldaux, None)


def test_linear_mxfp8_ex_rejects_bad_arguments():
    E = yvhip
    assert _lin(K=192, lda=192) == ERR_ARG                                      # K not a multiple of 128
    assert _lin(lda=264) == ERR_ARG                                             # misaligned operand stride
    assert _lin(ldo=250) == ERR_ARG                                             # misaligned output stride
    assert _lin(a_rows=200) == ERR_ARG                                          # scale rows not a multiple of 128
    assert _lin(flags=E.EPI_GELU | E.EPI_SAVE_PRE) == ERR_ARG                   # SAVE_PRE without aux
    assert _lin(flags=E.EPI_SAVE_PRE, aux=P, ldaux=256) == ERR_ARG              # SAVE_PRE needs GELU
    assert _lin(flags=E.EPI_GELU_BWD | E.EPI_GELU, aux=P, ldaux=256) == ERR_ARG  # GELU_BWD excludes GELU
    assert _lin(flags=E.EPI_GELU_BWD, aux=P, ldaux=250) == ERR_ARG              # misaligned aux stride
    assert _lin(flags=E.EPI_GELU_BWD | E.EPI_OUT_F32, aux=P, ldaux=256) == ERR_ARG  # trainer epilogues: bf16 output
    assert _lin(flags=0, res=P) == ERR_ARG                                      # residual source without RES_F32
    assert _lin(flags=E.EPI_GELU, aux=P, ldaux=256) == ERR_ARG                  # aux without an epilogue that uses it
    assert _lin(flags=512) == ERR_ARG                                           # the MX-output flag is not part of this API
    assert _lin(flags=E.EPI_SILU) == ERR_ARG                                    # unsupported epilogue
    assert _lin(flags=E.EPI_BIAS) == ERR_ARG                                    # bias flag without bias


def test_linear_mxfp8_instance_rule():
    E = yvhip
    f = yvhip.lib.yv_linear_mxfp8_instance
    assert f(6304, 2304, 768, E.EPI_BIAS) == 1                                  # ViT-B/16 bench shape, qkv forward
    assert f(6304, 3072, 768, E.EPI_BIAS | E.EPI_GELU | E.EPI_SAVE_PRE) == 1    # fc1 forward
    assert f(6304, 3072, 768, E.EPI_GELU_BWD) == 1                              # fc2 data gradient
    assert f(6304, 768, 768, E.EPI_BIAS | E.EPI_RES_F32) == 0                   # N = 768 products: 128 x 128 tiles
    assert f(12608, 768, 3072, E.EPI_BIAS | E.EPI_RES_F32) == 1                 # ... persistent from R = 64
    assert f(1000, 3072, 768, E.EPI_GELU_BWD) == 0                              # M < 2,048
    assert f(6304, 768, 768, E.EPI_SAVE_PRE) == ERR_ARG
    assert f(6304, 768, 100, 0) == ERR_ARG


def _wg(dy_ld=6400, x_ld=6400, T_pad=6400, N=768, K=768, ldw=768, dy_rows=768, x_rows=768):
    return yvhip.lib.yv_wgrad_mxfp8(P, dy_ld, P, dy_rows, P, x_ld, P, x_rows, T_pad, N, K, P, ldw, None)


def test_wgrad_mxfp8_rejects_bad_arguments():
    assert _wg(T_pad=6336, dy_ld=6336, x_ld=6336) == ERR_ARG    # T_pad not a multiple of 128
    assert _wg(dy_ld=6408) == ERR_ARG                           # misaligned operand stride
    assert _wg(x_ld=6272) == ERR_ARG                            # operand stride below T_pad
    assert _wg(ldw=770) == ERR_ARG                              # misaligned gradient row stride
    assert _wg(ldw=512) == ERR_ARG                              # gradient row stride below K
    assert _wg(dy_rows=700) == ERR_ARG                          # scale rows below N / not a multiple of 128
    assert _wg(N=764) == ERR_ARG                                # output width not a multiple of 8
    assert yvhip.lib.yv_wgrad_mxfp8(None, 6400, P, 768, P, 6400, P, 768, 6400, 768, 768, P, 768, None) == ERR_ARG


def test_trainer_recipe_rule(monkeypatch):
    from yvhip import training
    with pytest.raises(yvhip.YvError, match="dtype"):
        training.VitTrainer({}, "vit_tiny_test", dtype="fp8")
    with pytest.raises(yvhip.YvError, match="dtype"):
        training.check_train_dtype("mxfp4", 768)
    training.check_train_dtype("mxfp8", 768)
    training.check_train_dtype("bf16", 192)
    # a width that is not a multiple of 128 (ViT-Ti's 192): refused before any device work
    monkeypatch.setattr(training, "vit_cfg", lambda name: (16, 192, 12, 3))
    with pytest.raises(yvhip.YvError, match="multiple of 128"):
        training.VitTrainer({}, "vit_tiny_patch16_224", dtype="mxfp8")


def test_emulated_mx_linear_is_a_small_perturbation():
    """The emulation's three products stay within MX quantisation noise of the fp32 ones (and are not identical to them)."""
    from mx_train_emulation import MxLinear
    g = torch.Generator().manual_seed(3)
    x = torch.randn(300, 256, generator=g, requires_grad=True)
    w = (torch.randn(128, 256, generator=g) * 0.05).requires_grad_(True)
    b = torch.zeros(128, requires_grad=True)
    dy = torch.randn(300, 128, generator=g)
    y = MxLinear.apply(x, w, b)
    y.backward(dy)
    rel = lambda a, r: float((a - r).norm() / r.norm())
    for got, ref in ((y.detach(), x.detach() @ w.detach().t()), (x.grad, dy @ w.detach()), (w.grad, dy.t() @ x.detach())):
        assert 1e-3 < rel(got, ref) < 6e-2


def test_synthetic_task_is_learnable_by_the_fp32_oracle():
    import mx_train_emulation as m
    losses, acc = m.oracle_train_task(m.TASK_STEPS)
    print(f"oracle on the synthetic task: loss {losses[0]:.3f} -> {losses[-1]:.3f}, accuracy {acc:.2f} after {m.TASK_STEPS} steps")
    assert acc >= m.TASK_ACC
    assert losses[-1] <= m.TASK_LOSS_FRAC * losses[0]


def test_wrappers_check_caller_buffers():
    """The C ABI sees pointers and strides only: the Python wrappers refuse buffers of the wrong size or type before any device
    work (these are host tensors: a call that passed every size check would stop at the device check)."""
    u8, bf, f32 = torch.uint8, torch.bfloat16, torch.float32
    x = torch.zeros(100, 256, dtype=bf)
    for kw, msg in ((dict(q=torch.zeros(99, 256, dtype=u8)), "row form"),
                    (dict(q=torch.zeros(100, 256, dtype=bf)), "row form"),
                    (dict(scales=torch.zeros(2, 64, 4, dtype=u8)), "row form"),
                    (dict(qt=torch.zeros(128, 128, dtype=u8)), "column form"),
                    (dict(qt=torch.zeros(256, 100, dtype=u8)), "column form"),
                    (dict(scales_t=torch.zeros(1, 128, 4, dtype=u8)), "column form")):
        with pytest.raises(yvhip.YvError, match=msg):
            yvhip.quant_mxfp8_2d(x, **kw)
    with pytest.raises(yvhip.YvError, match="device"):
        yvhip.quant_mxfp8_2d(x)
    M, N, K = 300, 256, 256
    aq, asc = torch.zeros(M, K, dtype=u8), torch.zeros(K // 128, 384, 4, dtype=u8)
    wq, wsc = torch.zeros(N, K, dtype=u8), torch.zeros(K // 128, 256, 4, dtype=u8)
    lin = lambda **kw: yvhip.linear_mxfp8_ex(**{**dict(aq=aq, a_scale=asc, wq=wq, w_scale=wsc, bias=None,
                                                     out=torch.zeros(M, N, dtype=bf)), **kw})
    for kw, msg in ((dict(out=torch.zeros(M - 1, N, dtype=bf)), "out"),
                    (dict(out=torch.zeros(M, N, dtype=f32)), "out"),                                # bf16 output expected
                    (dict(out=torch.zeros(M, N, dtype=bf), flags=yvhip.EPI_RES_F32), "out"),       # f32 output expected
                    (dict(aux=torch.zeros(M, N - 8, dtype=bf), flags=yvhip.EPI_GELU_BWD), "aux"),
                    (dict(out=torch.zeros(M, N, dtype=f32), res_f32=torch.zeros(M, N + 8, dtype=f32)[:, :N],
                          flags=yvhip.EPI_RES_F32), "row stride"),
                    (dict(a_scale=torch.zeros(K // 128, 256, 4, dtype=u8)), "a_scale"),
                    (dict(wq=torch.zeros(N, K + 128, dtype=u8)), "wq"),
                    (dict(bias=torch.zeros(N - 8)), "bias")):
        with pytest.raises(yvhip.YvError, match=msg):
            lin(**kw)
    with pytest.raises(yvhip.YvError, match="device"):
        lin()
    dyt, xt = torch.zeros(768, 6400, dtype=u8), torch.zeros(768, 6400, dtype=u8)
    sc = torch.zeros(50, 768, 4, dtype=u8)
    with pytest.raises(yvhip.YvError, match="dw"):
        yvhip.wgrad_mxfp8(dyt, sc, xt, sc, torch.zeros(768, 640))
    with pytest.raises(yvhip.YvError, match="x_scale"):
        yvhip.wgrad_mxfp8(dyt, sc, xt, torch.zeros(49, 768, 4, dtype=u8), torch.zeros(768, 768))
    with pytest.raises(yvhip.YvError, match="device"):
        yvhip.wgrad_mxfp8(dyt, sc, xt, sc, torch.zeros(768, 768))


def test_cfg_train_dtype_reaches_the_trainer(monkeypatch):
    """utils.trainClass.fit -> module attribute -> _trainer_for -> VitTrainer(dtype=...), with a stand-in trainer: absent
    CFG.train_dtype keeps the bf16 default (no dtype argument at all), "mxfp8" builds an MX trainer, a change of recipe between
    two fits replaces the cached trainer, the same recipe reuses it, an unknown recipe is refused."""
    from utils import trainClass as tc
    from yvhip import training
    made = []

    class StubTrainer:
        def __init__(self, sd, name, nc, img, **kw):
            self.kw, self.dtype = kw, kw.get("dtype", "bf16")
            made.append(self)

    monkeypatch.setattr(training, "VitTrainer", StubTrainer)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 2)
            self.model = types.SimpleNamespace(arch="vit_tiny_test", img=224)
            self.num_class = 5

    net = Net()
    cfg = lambda **kw: types.SimpleNamespace(epoch=0, lr=0.01, **kw)
    tc.fit(net, None, None, cfg())
    t0 = tc._trainer_for(net, None)
    assert t0.dtype == "bf16" and "dtype" not in t0.kw
    tc.fit(net, None, None, cfg(train_dtype="mxfp8"))
    t1 = tc._trainer_for(net, None)
    assert t1 is not t0 and t1.kw["dtype"] == "mxfp8"
    tc.fit(net, None, None, cfg(train_dtype="mxfp8"))
    assert tc._trainer_for(net, None) is t1
    tc.fit(net, None, None, cfg())
    assert tc._trainer_for(net, None).dtype == "bf16" and len(made) == 3
    with pytest.raises(yvhip.YvError, match="dtype"):
        tc.fit(net, None, None, cfg(train_dtype="fp8"))
