"""CPU checks of the long-sequence attention backward (yv_attention_bwd_long, VitTrainer(long_attn_bwd=True)): the header /
binding agreement, host-side argument rejection (no GPU call is made: every case fails validation first, or asks for zero
crops), and the constructor argument."""
import ctypes as C
import inspect

import yvhip

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
POINTERS = ("qkv", "out", "dout", "lse", "dqkv", "delta_ws")


def _call(qkv=P, out=P, dout=P, lse=P, R=2, N=785, H=2, dqkv=P, delta_ws=P):
    return yvhip.lib.yv_attention_bwd_long(qkv, out, dout, lse, R, N, H, 0.125, dqkv, delta_ws, None)


def test_attention_bwd_long_is_declared_and_bound():
    assert "yv_attention_bwd_long" in yvhip.header_symbols()
    assert "yv_attention_bwd_long" in yvhip._SIGS
    assert "yv_attention_bwd_long" not in yvhip.MISSING
    assert callable(yvhip.attention_bwd_long)


def test_attention_bwd_long_rejects_bad_arguments():
    for name in POINTERS:
        assert _call(**{name: None}) == ERR_ARG, name
    for name in ("R", "N", "H"):                                               # negative sizes
        assert _call(**{name: -1}) == ERR_ARG, name
    assert _call(N=0) == ERR_ARG and _call(H=0) == ERR_ARG
    for name in ("qkv", "out", "dout", "dqkv"):                                # 16-byte aligned pointers
        assert _call(**{name: P + 8}) == ERR_ARG, name
    assert _call(R=1 << 30, N=1024, H=2) == ERR_LIMIT                          # more workgroups than a grid holds
    assert _call(R=0) == OK                                                    # nothing to do, nothing launched
    assert _call(R=0, N=1, H=1) == OK


def test_trainer_accepts_long_attn_bwd():
    from yvhip.training import VitTrainer
    assert inspect.signature(VitTrainer.__init__).parameters["long_attn_bwd"].default is None
