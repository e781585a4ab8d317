"""CPU checks of the FP8 attention (yv_attention_fp8, VitEngine(dtype="mxfp8", fp8_attn=True)): the numpy
statement against plain f64 attention, the header / binding agreement, host-side argument rejection (no GPU call is made: every
case fails validation first, or asks for zero crops), the K image's swizzle against the LDS lane groups of ds_read_b128, the
flag's parsing, and the launch trace of a flagged engine (tests/golden/engine_trace_fp8.json)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_fp8_reference as ref
import engine_trace
import engine_trace_fp8 as etf
import mx_reference as mxr
import yvhip
from yvhip import engines

OK, ERR_ARG, ERR_LIMIT = 0, -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced


# ------------------------------------------------------------------------------------------------ the statement
def device_scales(s_rows: torch.Tensor, rows_pad: int) -> torch.Tensor:
    """(rows, C / 32) scale bytes -> the K-step-major device layout (C / 128, rows_pad, 4)."""
    rows, kb = s_rows.shape
    s = torch.zeros((kb // 4, rows_pad, 4), dtype=torch.uint8)
    s[:, :rows] = s_rows.reshape(rows, kb // 4, 4).permute(1, 0, 2)
    return s


def quantised_qkv(R, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R * N, 3 * H * 64, generator=g) * torch.exp(torch.randn(R * N, 1, generator=g))).to(torch.bfloat16).float()
    q, s, d = mxr.emulate_quant(x)
    return q, device_scales(s, (R * N + 127) // 128 * 128), d


@pytest.mark.parametrize("R,N,H", [(1, 1, 2), (2, 3, 2), (1, 33, 4), (2, 70, 2)])
def test_statement_is_attention_of_the_decoded_operand(R, N, H):
    q, s, d = quantised_qkv(R, N, H, seed=R * 1000 + N)
    assert np.array_equal(ref.decode(q, s), d.numpy())                   # the layout round trip
    got = ref.attention_fp8(q, s, R, N, H, 0.125)
    x = d.reshape(R, N, 3, H, 64).permute(2, 0, 3, 1, 4)                  # (3, R, H, N, 64), f64
    want = (torch.softmax(x[0] @ x[1].transpose(-1, -2) * 0.125, -1) @ x[2]).permute(0, 2, 1, 3).reshape(R * N, H * 64)
    assert np.allclose(got["f64"], want.numpy(), rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    assert got["bf16"].dtype == torch.bfloat16
    assert float((got["bf16"].double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())      # half a bf16 step
    oq, os_ = mxr.emulate_quant_rows(got["bf16"].float())
    assert torch.equal(got["q"], oq) and torch.equal(got["s"], os_) and got["s"].shape == (R * N, 2 * H)


def test_statement_on_hand_sized_cases():
    # one token: the output is that token's V row, exactly
    q, s, d = quantised_qkv(2, 1, 2, seed=5)
    assert np.array_equal(ref.attention_fp8(q, s, 2, 1, 2, 0.125)["f64"], d[:, 256:].numpy())
    # a zero query: uniform probabilities, the mean of V
    q, s, d = quantised_qkv(1, 4, 2, seed=6)
    q[:, :128] = 0
    out = ref.attention_fp8(q, s, 1, 4, 2, 0.125)["f64"]
    assert np.allclose(out, np.broadcast_to(ref.decode(q, s)[:, 256:].mean(0), out.shape), rtol=1e-15, atol=0)
    # heads read their own scale bytes: doubling head 1's K scales changes head 1 only
    q, s, _ = quantised_qkv(1, 5, 2, seed=7)
    base = ref.attention_fp8(q, s, 1, 5, 2, 0.125)["f64"]
    s2 = s.clone()
    s2[1, :5, 2:4] += 1                                                    # K step 1 = K columns 0..127, bytes 2, 3 = head 1
    moved = ref.attention_fp8(q, s2, 1, 5, 2, 0.125)["f64"]
    assert np.array_equal(moved[:, :64], base[:, :64]) and not np.array_equal(moved[:, 64:], base[:, 64:])


def test_to_bf16_rounds_once_to_nearest_even():
    one, step = 1.0, 2.0 ** -7
    x = np.array([one + step / 2, one + 3 * step / 2, one + step / 2 + 2.0 ** -40, one + step / 2 - 2.0 ** -40, -one - step / 2, 0.0])
    assert ref.to_bf16(x).double().tolist() == [one, one + 2 * step, one + step, one, -one, 0.0]


# ------------------------------------------------------------------------------------------------ symbols and arguments
def test_symbols_are_declared_and_bound():
    vp, i, ll, f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    want = {"yv_attention_fp8": [vp, ll, vp, ll, i, i, i, f, vp, vp, vp, ll, vp, ll, vp],
            "yv_mx_probe32": [vp, vp, vp, vp, i, vp, vp],
            "yv_attention_fp8_dequant": [vp, ll, i, vp, vp]}
    for name, args in want.items():
        assert name in yvhip.header_symbols() and name not in yvhip.MISSING
        assert yvhip._SIGS[name] == (i, args)
        fn = getattr(yvhip.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args
    assert callable(yvhip.attention_fp8) and callable(yvhip.mx_probe32) and callable(yvhip.attention_fp8_dequant)


def _call(qkv_q=P, ld_in=384, qkv_scales=P, in_rows_pad=1664, R=2, N=785, H=2, out=P, r_dev=None, out_q=None, ldq=0,
          out_scales=None, rows_pad=0):
    return yvhip.lib.yv_attention_fp8(qkv_q, ld_in, qkv_scales, in_rows_pad, R, N, H, 0.125, out, r_dev, out_q, ldq, out_scales,
                                      rows_pad, None)


def _mx(**kw):
    a = dict(out=None, out_q=P, ldq=128, out_scales=P, rows_pad=1664)          # R * N = 1570 rows, padded to 13 * 128
    a.update(kw)
    return _call(**a)


def test_attention_fp8_rejects_bad_arguments():
    assert _call(qkv_q=None) == ERR_ARG and _call(qkv_scales=None) == ERR_ARG  # null pointers
    assert _call(out=None) == ERR_ARG                                          # one of out / out_q is required
    assert _call(out_q=P, ldq=128, rows_pad=1664) == ERR_ARG                   # out_q and out_scales come together
    assert _call(out_scales=P, ldq=128, rows_pad=1664) == ERR_ARG
    assert _call(out=None, out_scales=P, ldq=128, rows_pad=1664) == ERR_ARG
    for name in ("R", "N", "H"):
        assert _call(**{name: -1}) == ERR_ARG, name
    assert _call(N=0) == ERR_ARG and _call(H=0) == ERR_ARG
    assert _call(ld_in=383) == ERR_ARG and _call(ld_in=368) == ERR_ARG         # ld_in >= 3 * 64 H ...
    assert _call(ld_in=392) == ERR_ARG                                         # ... and a multiple of 16
    assert _call(in_rows_pad=1536) == ERR_ARG                                  # in_rows_pad >= R N
    assert _call(in_rows_pad=1600) == ERR_ARG                                  # in_rows_pad % 128 == 0
    assert _call(in_rows_pad=-128) == ERR_ARG
    assert _call(H=1, ld_in=192) == ERR_ARG and _call(H=3, ld_in=576) == ERR_ARG          # (64 H) % 128 == 0, with or without out_q
    assert _mx(H=1, ld_in=192, ldq=64) == ERR_ARG
    assert _call(qkv_q=P + 8) == ERR_ARG                                       # 16-byte aligned bytes and outputs
    assert _call(out=P + 2) == ERR_ARG
    assert _mx(out_q=P + 4) == ERR_ARG
    assert _mx(out=P + 8) == ERR_ARG
    assert _call(qkv_scales=P + 2) == ERR_ARG                                  # a row's K step of scales is one dword
    assert _mx(ldq=136) == ERR_ARG                                             # the out_q rules of yv_attention_long
    assert _mx(ldq=112) == ERR_ARG
    assert _mx(rows_pad=1600) == ERR_ARG
    assert _mx(rows_pad=1536) == ERR_ARG
    assert _mx(rows_pad=-128) == ERR_ARG
    assert _call(R=1 << 30, N=1024, H=2, in_rows_pad=1 << 40) == ERR_LIMIT     # more workgroups than a grid holds
    # nothing to do, nothing launched: every accepted combination with R = 0
    assert _call(R=0) == OK
    assert _call(R=0, N=1, in_rows_pad=0, ld_in=400) == OK
    assert _call(R=0, r_dev=P) == OK
    assert _mx(R=0, rows_pad=0) == OK
    assert _mx(R=0, out=P, ldq=256) == OK


def test_probe_and_dequant_reject_bad_arguments():
    lib = yvhip.lib
    for bad in range(5):
        args = [P, P, P, P, P]
        args[bad] = None
        assert lib.yv_mx_probe32(args[0], args[1], args[2], args[3], 0, args[4], None) == ERR_ARG
    assert lib.yv_mx_probe32(P, P, P, P, 4, P, None) == ERR_ARG and lib.yv_mx_probe32(P, P, P, P, -1, P, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(None, 256, 127, P, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(P, 256, 127, None, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(P, 0, 127, P, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(P, 254, 127, P, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(P, 256, 255, P, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(P, 256, -1, P, None) == ERR_ARG
    assert lib.yv_attention_fp8_dequant(P + 2, 256, 127, P, None) == ERR_ARG


def test_wrapper_checks_before_the_library():
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt)
    with pytest.raises(yvhip.YvError):
        yvhip.attention_fp8(z(4, 384), z(3, 128, 4), 1, 4, 2, out=z(4, 128, dt=torch.bfloat16))           # host tensors


# ------------------------------------------------------------------------------------------------ the K image's swizzle
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]


def k8_off(row, c):
    """csrc/attention_fwd_core.h: chunk c of row `row` of the K byte image."""
    return row * 64 + ((c ^ ((row >> 2) & 3)) << 4)


def test_k8_swizzle_is_conflict_free():
    """The A-fragment reads of score_group8 - lane (rl, hh) reads the 16-byte chunks hh and 2 + hh of row row0 + rl - against the
    16-lane groups of ds_read_b128 (a group is served in one LDS cycle when its 16 x 4 dwords fall on 64 distinct banks, bank =
    (address / 4) mod 64); and the image is a bijection of the tile."""
    groups = B128_GROUPS + [[l + 32 for l in g] for g in B128_GROUPS]
    for row0 in (0, 32):
        for second in (0, 2):
            for g in groups:
                banks = set()
                for lane in g:
                    a = k8_off(row0 + (lane & 31), second + (lane >> 5))
                    banks |= {((a >> 2) + i) % 64 for i in range(4)}
                assert len(banks) == 64, (row0, second, g)
    assert sorted(k8_off(r, c) for r in range(64) for c in range(4)) == list(range(0, 4096, 16))
    # the linear image is not: four rows of a group share each 64-byte quarter
    banks = {((r * 64 + 0) >> 2) % 64 for r in B128_GROUPS[0]}
    assert len(banks) == 4


# ------------------------------------------------------------------------------------------------ the flag
def _engine(monkeypatch, name, **kw):
    monkeypatch.setattr(engines, "require_gpu", lambda: None)
    monkeypatch.setattr(engines, "quant_mxfp8", lambda w: (w, w))
    return engines.VitEngine(engines.init_vit_wrapper_state(name, 5, seed=3), name, 5, device="cpu", **kw)


def test_flag_parsing(monkeypatch):
    monkeypatch.delenv(etf.VAR, raising=False)
    assert _engine(monkeypatch, etf.P16, dtype="mxfp8").fp8_attn is False            # default: off
    assert _engine(monkeypatch, etf.P16).fp8_attn is False
    assert _engine(monkeypatch, etf.P16, dtype="mxfp8", fp8_attn=True).fp8_attn is True
    with pytest.raises(yvhip.YvError, match="fp8_attn"):
        _engine(monkeypatch, etf.P16, fp8_attn=True)                                 # bf16 + the explicit flag
    with pytest.raises(yvhip.YvError, match="fp8_attn"):
        _engine(monkeypatch, etf.P16, dtype="bf16", fp8_attn=True)
    monkeypatch.setenv(etf.VAR, "1")
    assert _engine(monkeypatch, etf.P16, dtype="mxfp8").fp8_attn is True             # the variable turns it on ...
    assert _engine(monkeypatch, etf.P16).fp8_attn is False                           # ... a bf16 engine ignores it ...
    assert _engine(monkeypatch, etf.P16, dtype="mxfp8", fp8_attn=False).fp8_attn is False       # ... an argument overrides it
    monkeypatch.setenv(etf.VAR, "0")
    assert _engine(monkeypatch, etf.P16, dtype="mxfp8").fp8_attn is False


def test_flagged_engine_has_the_mx_qkv_buffers_and_no_bf16_qkv(monkeypatch):
    monkeypatch.delenv(etf.VAR, raising=False)
    e = _engine(monkeypatch, etf.P16, dtype="mxfp8", fp8_attn=True)
    b = e._buffers(3)
    assert "qkv" not in b
    assert b["qkv8"].dtype == torch.uint8 and tuple(b["qkv8"].shape) == (3 * 197, 384)
    assert b["qkv8s"].dtype == torch.uint8 and tuple(b["qkv8s"].shape) == (3, 768, 4)
    b = _engine(monkeypatch, etf.P16, dtype="mxfp8")._buffers(3)
    assert "qkv8" not in b and "qkv8s" not in b and b["qkv"].dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------ the launch trace
@pytest.fixture(scope="module")
def fixture():
    return etf.load_fixture()


def test_fixture_holds_exactly_the_cases(fixture):
    assert list(fixture) == list(etf.CASES)


@pytest.mark.parametrize("case", list(etf.CASES))
def test_trace_equals_fixture(fixture, case):
    got, want = etf.record_case(case), fixture[case]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{case}: call {i} differs\n  recorded: {g}\n  fixture:  {w}")
    assert len(got) == len(want)


@pytest.mark.parametrize("case", list(etf.CASES))
def test_trace_is_linear_q_then_attention_fp8_per_block(fixture, case):
    model, kw, _, with_count = etf.CASES[case]
    calls = fixture[case]
    L, N = engines.VIT_CFGS[model][2], 197 if model == etf.P16 else 785
    names = [c[0] for c in calls]
    # no other attention kernel, no quantisation pass, whatever long_attn and the token count say
    assert [n for n in names if n.startswith("attention") or n.startswith("quant_mxfp8")] == ["attention_fp8"] * L
    count = {"m_dev": "count"} if with_count else {}
    rcount = {"r_dev": "count"} if with_count else {}
    for i in range(L):
        at = [j for j, n in enumerate(names) if n == "attention_fp8"][i]
        prod, attn = calls[at - 1], calls[at]
        assert prod[0] == "linear_mxfp8_q"
        assert prod[2] == ["q", "qs", f"blocks.{i}.wqkv_q", f"blocks.{i}.wqkv_s", f"blocks.{i}.bqkv", "qkv8", "qkv8s"]
        assert prod[3] == {**count, "m_mul": N}
        assert attn[2] == ["qkv8", "qkv8s", engine_trace.CAP, N, 2]
        assert attn[3] == {**rcount, "out_q": "q", "out_scale": "qs"}
        assert names[at + 1] == "linear_mxfp8"                                       # proj reads what the attention wrote
    # per block: LayerNorm -> qkv (q), attention, proj, LayerNorm -> fc1 (q) -> fc2
    per_block = ["layernorm_mxfp8", "linear_mxfp8_q", "attention_fp8", "linear_mxfp8", "layernorm_mxfp8", "linear_mxfp8_q",
                 "linear_mxfp8"]
    body = [n for n in names if n in set(per_block)]
    assert body == per_block * L
    if kw.get("mid_gemm"):                                                           # the pass still runs inside the mid options
        opts = [c[2][0] for c in calls if c[0] == "set_option"]
        assert opts.count("linear_mx_mid") == 2 and opts.count("linear_mid") == 2


def test_flag_off_records_the_unflagged_engine(monkeypatch):
    """fp8_attn=False, or the variable on a bf16 engine: the calls of the engine without the argument."""
    base = etf.record(etf.P16, dict(dtype="mxfp8"), {})
    assert etf.record(etf.P16, dict(dtype="mxfp8", fp8_attn=False), {etf.VAR: "1"}) == base
    assert "attention_mxfp8" in [c[0] for c in base] and "attention_fp8" not in [c[0] for c in base]
    assert etf.record(etf.P16, dict(), {etf.VAR: "1"}) == etf.record(etf.P16, dict(), {})
