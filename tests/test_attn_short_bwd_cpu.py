"""CPU checks of the one-launch attention backward (yv_attention_bwd_short, VitTrainer(short_attn_bwd=True)): the header / binding
agreement, host-side argument rejection (no GPU call is made: every case fails validation first, or asks for zero crops), the
constructor argument and its precedence, CFG.train_short_attn_bwd on its way to the trainer, and the trainer's launch trace: the
fixture's trace with each attention_bwd call renamed, nothing else.  A workgroup takes one (crop, head) item, so there is no plan
function to test."""
import copy
import ctypes as C
import inspect
import types

import pytest
import torch

import trainer_trace as tt
import yvhip

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
POINTERS = ("qkv", "out", "dout", "lse", "dqkv", "delta_ws")


def _call(qkv=P, out=P, dout=P, lse=P, R=2, N=197, H=2, dqkv=P, delta_ws=P):
    return yvhip.lib.yv_attention_bwd_short(qkv, out, dout, lse, R, N, H, 0.125, dqkv, delta_ws, None)


def test_attention_bwd_short_is_declared_and_bound():
    assert "yv_attention_bwd_short" in yvhip.header_symbols()
    assert "yv_attention_bwd_short" in yvhip._SIGS
    assert yvhip._SIGS["yv_attention_bwd_short"] == yvhip._SIGS["yv_attention_bwd"]          # a drop-in at the call site
    assert "yv_attention_bwd_short" not in yvhip.MISSING
    assert callable(yvhip.attention_bwd_short)
    assert list(inspect.signature(yvhip.attention_bwd_short).parameters) == list(inspect.signature(yvhip.attention_bwd).parameters)


def test_attention_bwd_short_rejects_bad_arguments():
    for name in POINTERS:
        assert _call(**{name: None}) == ERR_ARG, name
    for name in ("R", "N", "H"):                                               # negative sizes
        assert _call(**{name: -1}) == ERR_ARG, name
    assert _call(N=0) == ERR_ARG and _call(H=0) == ERR_ARG
    for name in ("qkv", "out", "dout", "dqkv"):                                # 16-byte aligned pointers
        assert _call(**{name: P + 8}) == ERR_ARG, name
        assert _call(N=224, **{name: P + 8}) == ERR_ARG, name
    assert _call(N=225) == ERR_LIMIT and _call(N=785) == ERR_LIMIT             # the limit sits exactly at 224:
    assert _call(R=0, N=225) == ERR_LIMIT and _call(R=0, N=224) == OK          # N = 224 passes every check
    assert _call(R=1 << 20, N=197, H=1 << 11) == ERR_LIMIT                     # more workgroups than a grid holds
    assert _call(R=0) == OK                                                    # nothing to do, nothing launched
    assert _call(R=0, N=1, H=1) == OK


def test_trainer_accepts_short_attn_bwd():
    from yvhip.training import VitTrainer
    assert inspect.signature(VitTrainer.__init__).parameters["short_attn_bwd"].default is None


def test_flag_precedence(monkeypatch):
    """The argument beats the environment; unset means off; only "1" turns it on; the other flags do not move it."""
    from yvhip import engines
    from yvhip.training import VitTrainer
    tt._patch(monkeypatch, tt.Recorder())                      # the trainer is built on the CPU: nothing is launched
    sd = engines.init_vit_wrapper_state("vit_tiny_test", 5, seed=2)
    make = lambda **kw: VitTrainer(sd, "vit_tiny_test", 5, device="cpu", **kw)
    monkeypatch.delenv("YV_VIT_SHORT_ATTN_BWD", raising=False)
    monkeypatch.delenv("YV_VIT_LONG_ATTN_BWD", raising=False)
    assert make().short_attn_bwd is False and make(short_attn_bwd=True).short_attn_bwd is True
    assert make(short_attn_bwd=False).short_attn_bwd is False
    assert make(long_attn_bwd=True).short_attn_bwd is False and make(short_attn_bwd=True).long_attn_bwd is False
    monkeypatch.setenv("YV_VIT_SHORT_ATTN_BWD", "1")
    assert make().short_attn_bwd is True and make(short_attn_bwd=False).short_attn_bwd is False
    assert make(cls_tail=True, dtype="mxfp8").short_attn_bwd is True and make().long_attn_bwd is False
    monkeypatch.setenv("YV_VIT_SHORT_ATTN_BWD", "0")
    assert make().short_attn_bwd is False and make(short_attn_bwd=True).short_attn_bwd is True


def test_cfg_train_short_attn_bwd_reaches_the_trainer(monkeypatch):
    """utils.trainClass.fit -> module attribute -> _trainer_for -> VitTrainer(short_attn_bwd=True), with a stand-in trainer: absent
    or False passes no argument, True passes short_attn_bwd=True, a cached trainer of the other setting is replaced."""
    from utils import trainClass as tc
    from yvhip import training
    made = []

    class StubTrainer:
        def __init__(self, sd, name, nc, img, **kw):
            self.kw, self.dtype = kw, kw.get("dtype", "bf16")
            self.cls_tail, self.wide_wgrad = bool(kw.get("cls_tail", False)), bool(kw.get("wide_wgrad", False))
            self.short_attn_bwd = bool(kw.get("short_attn_bwd", False))
            made.append(self)

    monkeypatch.setattr(training, "VitTrainer", StubTrainer)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    for var in ("YV_VIT_TRAIN_CLS_TAIL", "YV_VIT_WIDE_WGRAD", "YV_VIT_SHORT_ATTN_BWD"):
        monkeypatch.delenv(var, raising=False)

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
    assert "short_attn_bwd" not in t0.kw and net._yv_train_short_attn_bwd is False
    tc.fit(net, None, None, cfg(train_short_attn_bwd=False))
    assert tc._trainer_for(net, None) is t0
    tc.fit(net, None, None, cfg(train_short_attn_bwd=True))
    t1 = tc._trainer_for(net, None)
    assert t1 is not t0 and t1.kw["short_attn_bwd"] is True
    assert not {"cls_tail", "dtype", "wide_wgrad"} & set(t1.kw)
    tc.fit(net, None, None, cfg(train_short_attn_bwd=True))
    assert tc._trainer_for(net, None) is t1
    tc.fit(net, None, None, cfg(train_short_attn_bwd=True, train_wide_wgrad=True))
    t2 = tc._trainer_for(net, None)
    assert t2 is not t1 and t2.kw == {**t2.kw, "short_attn_bwd": True, "wide_wgrad": True}
    tc.fit(net, None, None, cfg())
    t3 = tc._trainer_for(net, None)
    assert t3 is not t2 and "short_attn_bwd" not in t3.kw and len(made) == 4
    monkeypatch.setenv("YV_VIT_SHORT_ATTN_BWD", "1")           # the environment's trainer differs from the cached default one
    t4 = tc._trainer_for(net, None)
    assert t4 is not t3 and "short_attn_bwd" not in t4.kw


@pytest.mark.parametrize("case", ["bf16", "mxfp8_cls_tail"])
def test_trainer_trace_swaps_attention_bwd_for_attention_bwd_short(monkeypatch, case):
    """vit_tiny3_test (197 tokens) with short_attn_bwd=True records the fixture's case with every attention_bwd call named
    attention_bwd_short: same operands, same stream, same position; attention_cls_bwd and everything else unchanged."""
    monkeypatch.delenv("YV_VIT_SHORT_ATTN_BWD", raising=False)
    model, kw = tt.CASES[case]
    assert model == "vit_tiny3_test"
    monkeypatch.setitem(tt.CASES, case + "_short", (model, dict(kw, short_attn_bwd=True)))
    base, got = tt.load_fixture()[case], tt.record_case(case + "_short")
    assert got["allocs"] == base["allocs"]
    want, swapped = copy.deepcopy(base["calls"]), 0
    for c in want:
        if c[0] == "attention_bwd":
            c[0] = "attention_bwd_short"
            swapped += 1
    blocks = 3 - (1 if kw["cls_tail"] else 0)
    assert swapped == tt.STEPS * blocks and not any(c[0] == "attention_bwd_short" for c in base["calls"])
    assert got["calls"] == want
    assert not any(c[0] == "attention_bwd" for c in got["calls"])
    cls_bwd = lambda calls: [c for c in calls if c[0] == "attention_cls_bwd"]
    assert cls_bwd(got["calls"]) == cls_bwd(base["calls"]) and len(cls_bwd(got["calls"])) == tt.STEPS * (3 - blocks)


def test_trainer_trace_of_a_long_sequence_model_ignores_the_flag(monkeypatch):
    """vit_tiny3p8_test (785 tokens): accepted, not effective - the fixture's "bf16_p8_long" case call for call."""
    monkeypatch.delenv("YV_VIT_SHORT_ATTN_BWD", raising=False)
    model, kw = tt.CASES["bf16_p8_long"]
    assert model == "vit_tiny3p8_test" and kw["long_attn"] and kw["long_attn_bwd"]
    monkeypatch.setitem(tt.CASES, "bf16_p8_long_short", (model, dict(kw, short_attn_bwd=True)))
    base, got = tt.load_fixture()["bf16_p8_long"], tt.record_case("bf16_p8_long_short")
    assert got == base
    assert any(c[0] == "attention_bwd_long" for c in got["calls"])
    assert not any(c[0] == "attention_bwd_short" for c in got["calls"])
