"""CPU checks of the long-sequence attention forward (yv_attention_long, VitEngine(long_attn=True)): the header / binding
agreement, host-side argument rejection (no GPU call is made: every case fails validation first, or asks for zero crops), and
which attention launcher the classifier's block loop calls, with recorders in place of the launchers."""
import ctypes as C

import pytest
import torch

import yvhip
from yvhip import engines

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced


def _call(qkv=P, R=2, N=785, H=2, out=P, r_dev=None, lse=None, out_q=None, ldq=0, out_scales=None, rows_pad=0):
    return yvhip.lib.yv_attention_long(qkv, R, N, H, 0.125, out, r_dev, lse, out_q, ldq, out_scales, rows_pad, None)


def _mx(**kw):
    a = dict(out=None, out_q=P, ldq=128, out_scales=P, rows_pad=1664)          # R * N = 1570 rows, padded to 13 * 128
    a.update(kw)
    return _call(**a)


def test_attention_long_is_declared_and_bound():
    assert "yv_attention_long" in yvhip.header_symbols()
    assert "yv_attention_long" in yvhip._SIGS
    assert "yv_attention_long" not in yvhip.MISSING
    assert callable(yvhip.attention_long)


def test_attention_long_rejects_bad_arguments():
    assert _call(qkv=None) == ERR_ARG
    assert _call(out=None) == ERR_ARG                                          # one of out / out_q is required
    assert _call(out_q=P, ldq=128, rows_pad=1664) == ERR_ARG                   # out_q and out_scales come together
    assert _call(out_scales=P, ldq=128, rows_pad=1664) == ERR_ARG
    assert _call(out=None, out_scales=P, ldq=128, rows_pad=1664) == ERR_ARG
    for name in ("R", "N", "H"):                                               # negative sizes
        assert _call(**{name: -1}) == ERR_ARG, name
    assert _call(N=0) == ERR_ARG and _call(H=0) == ERR_ARG
    assert _mx(H=1, ldq=64) == ERR_ARG                                         # the MX image: H even
    assert _mx(H=3, ldq=192) == ERR_ARG
    assert _mx(ldq=136) == ERR_ARG                                             # ldq % 16 == 0
    assert _mx(ldq=112) == ERR_ARG                                             # ldq >= 64 H
    assert _mx(rows_pad=1600) == ERR_ARG                                       # rows_pad % 128 == 0
    assert _mx(rows_pad=1536) == ERR_ARG                                       # rows_pad >= R N
    assert _mx(rows_pad=-128) == ERR_ARG
    assert _call(qkv=P + 8) == ERR_ARG                                         # 16-byte aligned pointers
    assert _call(out=P + 2) == ERR_ARG
    assert _mx(out_q=P + 4) == ERR_ARG
    assert _mx(out=P + 8) == ERR_ARG
    assert _call(R=1 << 30, N=1024, H=2) == ERR_LIMIT                          # more workgroups than a grid holds
    # nothing to do, nothing launched: every accepted combination of outputs with R = 0
    assert _call(R=0) == OK
    assert _call(R=0, N=1, H=1) == OK
    assert _call(R=0, lse=P, r_dev=P) == OK
    assert _mx(R=0, rows_pad=0) == OK
    assert _mx(R=0, out=P, lse=P, ldq=256) == OK


# ------------------------------------------------------------------------------------------------ which launcher
def _stub_launchers(monkeypatch):
    """Recorders for the three attention launchers of the block loop; every other launcher does nothing."""
    ev = []
    for fn in ("cls_rows", "layernorm", "linear", "linear_res_ln", "layernorm_mxfp8", "linear_mxfp8", "linear_mxfp8_q",
               "quant_mxfp8"):
        monkeypatch.setattr(engines, fn, lambda *a, **k: None)
    monkeypatch.setattr(engines, "attention", lambda *a, **k: ev.append(("attention", k)))
    monkeypatch.setattr(engines, "attention_mxfp8", lambda *a, **k: ev.append(("attention_mxfp8", k)))
    monkeypatch.setattr(engines, "attention_cls", lambda *a, **k: ev.append(("attention_cls", k)))
    monkeypatch.setattr(engines, "attention_long", lambda *a, **k: ev.append(("attention_long", k)))
    return ev


def _engine(monkeypatch, name, **kw):
    """A real VitEngine (its constructor, its switches) on CPU tensors: no device is asked for, the weight quantiser is a stub."""
    monkeypatch.setattr(engines, "require_gpu", lambda: None)
    monkeypatch.setattr(engines, "quant_mxfp8", lambda w: (w, w))
    return engines.VitEngine(engines.init_vit_wrapper_state(name, 5, seed=3), name, 5, device="cpu", **kw)


def _run(monkeypatch, eng, cap=2):
    ev = _stub_launchers(monkeypatch)
    eng._backbone_pass(eng.patch_buffer(cap), cap, None, 0)
    return ev


@pytest.mark.parametrize("fused_ln", [False, True])
@pytest.mark.parametrize("cls_tail", [True, False])
def test_long_attn_engine_calls_attention_long(monkeypatch, cls_tail, fused_ln):
    monkeypatch.delenv("YV_VIT_LONG_ATTN", raising=False)
    eng = _engine(monkeypatch, "vit_tiny8_test", long_attn=True, cls_tail=cls_tail, fused_ln=fused_ln)
    assert eng.long_attn and eng.N == 785
    names = [e[0] for e in _run(monkeypatch, eng)]
    # every block but the cls-tail block; attention_cls of the tail is unchanged; attention is never called
    assert names == (["attention_long"] * (eng.L - 1) + ["attention_cls"] if cls_tail else ["attention_long"] * eng.L)


def test_long_attn_engine_mxfp8_writes_the_proj_operand(monkeypatch):
    monkeypatch.delenv("YV_VIT_LONG_ATTN", raising=False)
    eng = _engine(monkeypatch, "vit_tiny8_test", long_attn=True, dtype="mxfp8")
    ev = _run(monkeypatch, eng)
    assert [e[0] for e in ev] == ["attention_long"] * eng.L                    # never attention_mxfp8, never attention
    b = eng._buffers(2)
    for _, k in ev:
        assert k["out_q"] is b["q"] and k["out_scale"] is b["qs"]


def test_long_attn_is_not_effective_at_short_sequences(monkeypatch):
    monkeypatch.delenv("YV_VIT_LONG_ATTN", raising=False)
    eng = _engine(monkeypatch, "vit_tiny_test", long_attn=True)                # 197 tokens: the flag is accepted ...
    assert eng.long_attn and eng.N == 197
    assert [e[0] for e in _run(monkeypatch, eng)] == ["attention", "attention_cls"]          # ... and attention is kept
    eng = _engine(monkeypatch, "vit_tiny_test", long_attn=True, dtype="mxfp8")
    assert [e[0] for e in _run(monkeypatch, eng)] == ["attention_mxfp8"] * 2


def test_long_attn_default_and_environment(monkeypatch):
    monkeypatch.delenv("YV_VIT_LONG_ATTN", raising=False)
    eng = _engine(monkeypatch, "vit_tiny8_test")                               # default: off
    assert eng.long_attn is False
    assert [e[0] for e in _run(monkeypatch, eng)] == ["attention", "attention_cls"]
    eng = _engine(monkeypatch, "vit_tiny8_test", dtype="mxfp8")
    assert [e[0] for e in _run(monkeypatch, eng)] == ["attention_mxfp8"] * 2
    monkeypatch.setenv("YV_VIT_LONG_ATTN", "1")                                # the variable turns it on ...
    eng = _engine(monkeypatch, "vit_tiny8_test")
    assert eng.long_attn is True
    assert [e[0] for e in _run(monkeypatch, eng)] == ["attention_long", "attention_cls"]
    assert _engine(monkeypatch, "vit_tiny8_test", dtype="mxfp8").long_attn is True
    assert _engine(monkeypatch, "vit_tiny8_test", long_attn=False).long_attn is False       # ... an argument overrides it


def test_trainer_accepts_long_attn():
    import inspect
    from yvhip.training import VitTrainer
    assert inspect.signature(VitTrainer.__init__).parameters["long_attn"].default is None
