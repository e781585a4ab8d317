"""CPU checks of the fused residual + LayerNorm GEMM (yv_linear_res_ln, VitEngine(fused_ln=True)): host-side argument
rejection (no GPU call is made: every case fails validation first, or asks for zero rows), the header / binding agreement, and
the launch sequence of the classifier's block loop with recorders in place of the launchers."""
import ctypes as C

import pytest
import torch

import yvhip
from yvhip import engines

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced


def _call(a=P, lda=None, w=P, bias=P, M=8, N=768, K=768, x=P, ldx=None, gamma=P, beta=P, h=P, ldh=None, m_dev=None):
    return yvhip.lib.yv_linear_res_ln(a, K if lda is None else lda, w, bias, M, N, K, x, N if ldx is None else ldx, gamma, beta,
                                      1e-6, h, N if ldh is None else ldh, m_dev, 1, None)


def test_linear_res_ln_rejects_bad_arguments():
    for name in ("a", "w", "bias", "x", "gamma", "beta", "h"):                 # null operands
        assert _call(**{name: None}) == ERR_ARG, name
    assert _call(N=200) == ERR_ARG                                             # a width without an instance
    assert _call(N=256) == ERR_ARG
    assert _call(K=96) == ERR_ARG                                              # K below 128 / not a multiple of 64
    assert _call(K=100) == ERR_ARG
    assert _call(K=160) == ERR_ARG
    assert _call(ldx=5) == ERR_ARG                                             # strides: multiples of 8 that cover the row
    assert _call(lda=772) == ERR_ARG
    assert _call(ldh=780) == ERR_ARG
    assert _call(ldx=760) == ERR_ARG
    assert _call(lda=760) == ERR_ARG
    assert _call(M=-1) == ERR_ARG
    assert _call(x=P + 8) == ERR_ARG                                           # 16-byte chunks
    assert _call(h=P + 4) == ERR_ARG
    assert _call(M=1 << 20, N=1024, K=1024) == ERR_LIMIT                       # 32-bit byte offsets
    for N in yvhip.RES_LN_WIDTHS:
        assert _call(M=0, N=N, K=128) == OK                                    # nothing to do, nothing launched
    assert yvhip.RES_LN_WIDTHS == (128, 768, 1024)


def test_linear_res_ln_is_declared_and_bound():
    assert "yv_linear_res_ln" in yvhip.header_symbols()
    assert "yv_linear_res_ln" in yvhip._SIGS
    assert "yv_linear_res_ln" not in yvhip.MISSING
    assert callable(yvhip.linear_res_ln)


# ------------------------------------------------------------------------------------------------ launch plan
D_, TOK_, H_ = 128, 4, 2


def _engine(L, cls_tail, fused_ln):
    """A VitEngine without its device parts: tags in place of parameters, CPU activation buffers."""
    e = object.__new__(engines.VitEngine)
    e.dtype, e.cls_tail, e.fused_ln = "bf16", cls_tail, fused_ln
    e.P, e.D, e.L, e.H = 16, D_, L, H_
    e.tok, e.N, e.dev = TOK_, TOK_ + 1, torch.device("cpu")
    e.w_pe, e.b_pe, e.cls, e.pos = "w_pe", "b_pe", "cls", "pos"
    e.blocks = [{k: f"{k}{i}" for k in ("n1w", "n1b", "wqkv", "bqkv", "wproj", "bproj", "n2w", "n2b", "wfc1", "bfc1", "wfc2",
                                        "bfc2")} for i in range(L)]
    e.blocks[-1].update({k: f"{k}{L - 1}" for k in ("wq", "bq", "wkv", "bkv")})
    e.nw, e.nb, e.w_head, e.b_head = "nw", "nb", "w_head", "b_head"
    e._bufs, e._guards, e.full_cus_from = {}, {}, None
    return e


def _record(monkeypatch, eng, cap=2):
    ev = []
    monkeypatch.setattr(engines, "cls_rows", lambda *a, **k: None)
    monkeypatch.setattr(engines, "attention", lambda *a, **k: ev.append(("attention",)))
    monkeypatch.setattr(engines, "attention_cls", lambda *a, **k: ev.append(("attention_cls",)))
    monkeypatch.setattr(engines, "layernorm", lambda x, gamma, beta, y, *a, **k: ev.append(("layernorm", gamma, beta)))
    monkeypatch.setattr(engines, "linear",
                        lambda a, w, bias, out, flags=0, **k: ev.append(("linear", w, bias, bool(flags & yvhip.EPI_RES_F32))))
    monkeypatch.setattr(engines, "linear_res_ln",
                        lambda a, w, bias, x, gamma, beta, h, **k: ev.append(("linear_res_ln", w, bias, gamma, beta)))
    patches = torch.zeros(cap * TOK_, 3 * 16 * 16, dtype=torch.bfloat16)
    eng._backbone_pass(patches, cap, None, 0)
    return ev


def _expected(L, cls_tail, fused):
    """The sequence of VitEngine's block loop, written out from its description."""
    ev = [("linear", "w_pe", "b_pe", False)]
    full = L - 1 if cls_tail else L
    for i in range(full):
        if not fused or i == 0:
            ev.append(("layernorm", f"n1w{i}", f"n1b{i}"))
        ev += [("linear", f"wqkv{i}", f"bqkv{i}", False), ("attention",)]
        if fused:
            ev.append(("linear_res_ln", f"wproj{i}", f"bproj{i}", f"n2w{i}", f"n2b{i}"))
        else:
            ev += [("linear", f"wproj{i}", f"bproj{i}", True), ("layernorm", f"n2w{i}", f"n2b{i}")]
        ev.append(("linear", f"wfc1{i}", f"bfc1{i}", False))
        if fused and i + 1 < L:
            ev.append(("linear_res_ln", f"wfc2{i}", f"bfc2{i}", f"n1w{i + 1}", f"n1b{i + 1}"))
        else:
            ev.append(("linear", f"wfc2{i}", f"bfc2{i}", True))
    if cls_tail:
        i = L - 1
        if not fused or i == 0:
            ev.append(("layernorm", f"n1w{i}", f"n1b{i}"))
        ev += [("linear", f"wkv{i}", f"bkv{i}", False), ("linear", f"wq{i}", f"bq{i}", False), ("attention_cls",),
               ("linear", f"wproj{i}", f"bproj{i}", True), ("layernorm", f"n2w{i}", f"n2b{i}"),
               ("linear", f"wfc1{i}", f"bfc1{i}", False), ("linear", f"wfc2{i}", f"bfc2{i}", True)]
    ev += [("layernorm", "nw", "nb"), ("linear", "w_head", "b_head", False)]
    return ev


@pytest.mark.parametrize("cls_tail", [True, False])
@pytest.mark.parametrize("L", [2, 12])
def test_vit_block_launch_plan(monkeypatch, L, cls_tail):
    fused = _record(monkeypatch, _engine(L, cls_tail, True))
    assert fused == _expected(L, cls_tail, True)
    n_ln = sum(e[0] == "layernorm" for e in fused)
    assert n_ln == (3 if cls_tail else 2)
    # every proj of a full block carries its block's norm2, every fc2 but the last block's the next block's norm1
    full = L - 1 if cls_tail else L
    rl = [e for e in fused if e[0] == "linear_res_ln"]
    assert [e for e in rl if e[1].startswith("wproj")] == [("linear_res_ln", f"wproj{i}", f"bproj{i}", f"n2w{i}", f"n2b{i}")
                                                          for i in range(full)]
    assert [e for e in rl if e[1].startswith("wfc2")] == [("linear_res_ln", f"wfc2{i}", f"bfc2{i}", f"n1w{i + 1}", f"n1b{i + 1}")
                                                         for i in range(min(full, L - 1))]
    # off: today's sequence, no fused launch, 2L + 1 LayerNorms
    plain = _record(monkeypatch, _engine(L, cls_tail, False))
    assert plain == _expected(L, cls_tail, False)
    assert not any(e[0] == "linear_res_ln" for e in plain)
    assert sum(e[0] == "layernorm" for e in plain) == 2 * L + 1
