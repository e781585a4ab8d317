"""CPU checks of the trainer's cls-row tail (yv_attention_cls_train, yv_attention_cls_bwd, VitTrainer(cls_tail=True)): the
header / binding agreement, host-side argument rejection (no GPU call is made: every case fails validation first, or asks for zero
crops), the constructor argument, and CFG.train_cls_tail's way from fit() to the trainer."""
import ctypes as C
import inspect
import types

import torch

import yvhip

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
ENTRIES = ("yv_attention_cls_train", "yv_attention_cls_bwd")


def _fwd(q=P, ldq=128, qkv=P, R=2, N=197, H=2, out=P, lse=P):
    return yvhip.lib.yv_attention_cls_train(q, ldq, qkv, R, N, H, 0.125, out, lse, None)


def _bwd(q=P, ldq=128, qkv=P, dout=P, lse=P, R=2, N=197, H=2, dqkv=P):
    return yvhip.lib.yv_attention_cls_bwd(q, ldq, qkv, dout, lse, R, N, H, 0.125, dqkv, None)


CALLS = ((_fwd, ("q", "qkv", "out", "lse"), ("q", "qkv", "out")), (_bwd, ("q", "qkv", "dout", "lse", "dqkv"), ("q", "qkv", "dout", "dqkv")))


def test_entries_are_declared_and_bound():
    for name in ENTRIES:
        assert name in yvhip.header_symbols()
        assert name in yvhip._SIGS
        assert name not in yvhip.MISSING
    assert callable(yvhip.attention_cls_train) and callable(yvhip.attention_cls_bwd)


def test_entries_reject_bad_arguments():
    for call, pointers, aligned16 in CALLS:
        for name in pointers:
            assert call(**{name: None}) == ERR_ARG, name
        for name in ("R", "N", "H"):                                           # negative sizes
            assert call(**{name: -1}) == ERR_ARG, name
        assert call(N=0) == ERR_ARG and call(H=0) == ERR_ARG
        for name in aligned16:                                                 # 16-byte aligned operands
            assert call(**{name: P + 8}) == ERR_ARG, name
        assert call(ldq=132) == ERR_ARG                                        # q's row stride: whole 16-byte chunks ...
        assert call(ldq=64) == ERR_ARG                                         # ... and at least H * 64 elements
        assert call(ldq=0) == ERR_ARG
        assert call(N=8193) == ERR_LIMIT                                       # one query's scores live in LDS
        assert call(R=1 << 30, H=4, ldq=256) == ERR_LIMIT                      # more workgroups than a grid holds
        assert call(N=8192, R=0) == OK                                         # nothing to do, nothing launched
        assert call(R=0) == OK and call(R=0, N=1, H=1, ldq=64) == OK
        assert call(R=0, ldq=197 * 3 * 128) == OK                              # the trainer's stride: row r*N of the qkv buffer


def test_trainer_accepts_cls_tail():
    from yvhip.training import VitTrainer
    assert inspect.signature(VitTrainer.__init__).parameters["cls_tail"].default is None


def test_cfg_train_cls_tail_reaches_the_trainer(monkeypatch):
    """utils.trainClass.fit -> module attribute -> _trainer_for -> VitTrainer(cls_tail=True), with a stand-in trainer: an absent
    (or False) CFG.train_cls_tail passes no argument, True passes cls_tail=True, a cached trainer of the other setting is replaced,
    one of the same setting is reused; the recipe travels independently."""
    from utils import trainClass as tc
    from yvhip import training
    made = []

    class StubTrainer:
        def __init__(self, sd, name, nc, img, **kw):
            self.kw, self.dtype, self.cls_tail = kw, kw.get("dtype", "bf16"), bool(kw.get("cls_tail", False))
            made.append(self)

    monkeypatch.setattr(training, "VitTrainer", StubTrainer)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.delenv("YV_VIT_TRAIN_CLS_TAIL", raising=False)

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
    assert "cls_tail" not in t0.kw and net._yv_train_cls_tail is False
    tc.fit(net, None, None, cfg(train_cls_tail=False))
    assert tc._trainer_for(net, None) is t0
    tc.fit(net, None, None, cfg(train_cls_tail=True))
    t1 = tc._trainer_for(net, None)
    assert t1 is not t0 and t1.kw["cls_tail"] is True and "dtype" not in t1.kw
    tc.fit(net, None, None, cfg(train_cls_tail=True))
    assert tc._trainer_for(net, None) is t1
    tc.fit(net, None, None, cfg(train_cls_tail=True, train_dtype="mxfp8"))
    t2 = tc._trainer_for(net, None)
    assert t2 is not t1 and t2.kw == {**t2.kw, "cls_tail": True, "dtype": "mxfp8"}
    tc.fit(net, None, None, cfg())
    t3 = tc._trainer_for(net, None)
    assert t3 is not t2 and "cls_tail" not in t3.kw and "dtype" not in t3.kw and len(made) == 4
