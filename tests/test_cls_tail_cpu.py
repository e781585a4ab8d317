"""CPU checks of the cls-row tail of the classifier's last block: host-side argument rejection of yv_attention_cls (no GPU
call is made: every case fails validation first, or asks for zero crops) and the header / binding agreement."""
import ctypes as C

import yvhip

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced


def _att(q=P, qkv=P, R=2, N=197, H=12, out=P, r_dev=None):
    return yvhip.lib.yv_attention_cls(q, qkv, R, N, H, 0.125, out, r_dev, None)


def test_attention_cls_rejects_bad_arguments():
    assert _att(q=None) == ERR_ARG                               # null operands
    assert _att(qkv=None) == ERR_ARG
    assert _att(out=None) == ERR_ARG
    assert _att(R=-1) == ERR_ARG                                 # bad shapes
    assert _att(N=0) == ERR_ARG
    assert _att(N=-5) == ERR_ARG
    assert _att(H=0) == ERR_ARG
    assert _att(q=P + 8) == ERR_ARG                              # 16-byte row chunks: misaligned operands
    assert _att(qkv=P + 2) == ERR_ARG
    assert _att(out=P + 4) == ERR_ARG
    assert _att(N=8193) == ERR_LIMIT                             # the scores of one query live in LDS
    assert _att(R=1 << 30, H=16) == ERR_LIMIT                    # grid size
    assert _att(R=0) == OK                                       # nothing to do, nothing launched


def test_attention_cls_is_declared_and_bound():
    assert "yv_attention_cls" in yvhip.header_symbols()
    assert "yv_attention_cls" in yvhip._SIGS
    assert sorted(yvhip._SIGS) == yvhip.header_symbols()
    assert "yv_attention_cls" not in yvhip.MISSING
    assert callable(yvhip.attention_cls)


def test_skinny_option_is_known():
    assert yvhip.get_option("linear_skinny") == 256
    yvhip.set_option("linear_skinny", 0)
    try:
        assert yvhip.get_option("linear_skinny") == 0
        # options are process-wide, except "linear_p8_cus": it belongs to the thread that set it
        import threading
        seen = {}
        other = threading.Thread(target=lambda: seen.update(cus=yvhip.get_option("linear_p8_cus"),
                                                            skinny=yvhip.get_option("linear_skinny")))
        yvhip.set_option("linear_p8_cus", 96)
        try:
            assert yvhip.get_option("linear_p8_cus") == 96
            other.start()
            other.join()
        finally:
            yvhip.set_option("linear_p8_cus", 0)
        assert seen == {"cus": 0, "skinny": 0}
    finally:
        yvhip.set_option("linear_skinny", 256)
