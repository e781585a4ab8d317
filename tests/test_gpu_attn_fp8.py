"""GPU checks of the FP8 attention (yv_attention_fp8, VitEngine(dtype="mxfp8", fp8_attn=True)): the operand
layout of v_mfma_scale_f32_32x32x64_f8f6f4 measured and pinned; the V dequantisation over every e4m3 byte; on operands whose
scores are exact in f32 the bytes of yv_attention_long run on the dequantised bf16 copy, over every blocking edge; random data
against yv_attention_long and the f64 statement (attn_fp8_reference.py); the producer's bytes; the flagged engine against a
hand-run chain, the fp32 oracle and the bf16 engine."""
import functools

import numpy as np
import pytest
import torch

import attn_fp8_reference as ref
import mx_reference as mxr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE = 0x38                                               # 1.0 in e4m3


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def r128(n):
    return (n + 127) // 128 * 128


def device_scales(s_rows: torch.Tensor, rows_pad: int) -> torch.Tensor:
    """(rows, C / 32) scale bytes -> the K-step-major device layout (C / 128, rows_pad, 4)."""
    rows, kb = s_rows.shape
    s = torch.zeros((kb // 4, rows_pad, 4), dtype=torch.uint8)
    s[:, :rows] = s_rows.reshape(rows, kb // 4, 4).permute(1, 0, 2)
    return s


# ------------------------------------------------------------------------------------------------ 1. the MFMA's operand layout
def test_mx_mfma32_layout(yv):
    """Executable statement of the v_mfma_scale_f32_32x32x64_f8f6f4 operand layout score_group8 relies on, measured first and then
    compared with the statement (the values measured are printed).  Lane l = (row / column l & 31, half l >> 5); slot (h, b) = byte
    b of the 32 bytes of a lane of half h.
      * pairing: the A slot (h, b) of a row meets the B slot (h, b) of a column - the same half, the same byte: one-hot B against
        an A row of 64 distinct values;
      * blocks: bytes 0..15 of both halves are the MX block 0 (k = 0..31), bytes 16..31 block 1 (k = 32..63): inside a block the
        statement numbers k = 16 h + (b & 15), an order no product can observe;
      * scales: of the 64 scale registers only those of lanes r and r + 32 reach row r; lane (r, half j) carries block j's, in
        byte `opsel`; the same for B's columns."""
    def run(a, b, sa, sb, opsel=0):
        d = yv.mx_probe32(a.to(DEV), b.to(DEV), sa.to(DEV), sb.to(DEV), opsel)
        torch.cuda.synchronize()
        return d.cpu()

    def mat(d):                                          # (64 lanes, 16 registers) -> D[row][col], the C/D layout of 32x32x16
        lane, reg = torch.arange(64)[:, None], torch.arange(16)[None, :]
        m = torch.zeros(32, 32)
        m[(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), (lane & 31).expand(64, 16)] = d
        return m
    ones = lambda: torch.full((64, 32), ONE, dtype=torch.uint8)
    zeros = lambda: torch.zeros((64, 32), dtype=torch.uint8)
    s127 = lambda: torch.full((64,), 127, dtype=torch.int32)
    assert mat(run(ones(), ones(), s127(), s127())).unique().tolist() == [64.0]
    r, c = 5, 19
    # -- pairing: A row r holds the code 0x08 + slot in slot 32 h + b; B column c is one-hot
    a = zeros()
    for h in range(2):
        a[32 * h + r] = torch.arange(32, dtype=torch.uint8) + 0x08 + 32 * h
    value = (torch.arange(64, dtype=torch.uint8) + 0x08).view(torch.float8_e4m3fn).float()
    assert value.unique().numel() == 64
    pair = {}
    for h in range(2):
        for bb in range(32):
            b = zeros(); b[32 * h + c, bb] = ONE
            m = mat(run(a, b, s127(), s127()))
            hit = (value == m[r, c]).nonzero().flatten().tolist()
            assert len(hit) == 1 and int((m != 0).sum()) == 1, (h, bb, m[r, c])
            pair[(h, bb)] = divmod(hit[0], 32)
    print("B slot (half, byte) -> A slot (half, byte):", pair)
    assert all(k == v for k, v in pair.items())
    # -- which scale registers reach row r (A) / column c (B)
    a = zeros(); a[r] = ONE; a[32 + r] = ONE             # row r all ones: D[r][*] = 64
    b = zeros(); b[c] = ONE; b[32 + c] = ONE
    reach_a, reach_b = {}, {}
    for lane in range(64):
        s = s127(); s[lane] = 128
        v = mat(run(a, ones(), s, s127()))[r].unique().tolist()
        if v != [64.0]:
            reach_a[lane] = v
        v = mat(run(ones(), b, s127(), s))[:, c].unique().tolist()
        if v != [64.0]:
            reach_b[lane] = v
    print("scale lanes that reach row", r, ":", reach_a, "; column", c, ":", reach_b)
    assert reach_a == {r: [96.0], r + 32: [96.0]} and reach_b == {c: [96.0], c + 32: [96.0]}
    # -- which bytes each of the two carries: 16 bytes of one lane at a time
    block_a, block_b = {}, {}
    for h in range(2):
        for k2 in range(2):
            a = zeros(); a[32 * h + r, 16 * k2:16 * k2 + 16] = ONE
            b = zeros(); b[32 * h + c, 16 * k2:16 * k2 + 16] = ONE
            for j in range(2):
                s = s127(); s[32 * j + r] = 128
                va = mat(run(a, ones(), s, s127()))
                assert va[r].unique().numel() == 1 and float(va.sum()) == float(va[r].sum())
                s = s127(); s[32 * j + c] = 128
                vb = mat(run(ones(), b, s127(), s))
                assert vb[:, c].unique().numel() == 1 and float(vb.sum()) == float(vb[:, c].sum())
                assert float(va[r, 0]) in (16.0, 32.0) and float(vb[0, c]) in (16.0, 32.0)
                if float(va[r, 0]) == 32.0:
                    block_a.setdefault((h, k2), []).append(j)
                if float(vb[0, c]) == 32.0:
                    block_b.setdefault((h, k2), []).append(j)
    print("(half, 16-byte part) -> scale lane half, A:", block_a, " B:", block_b)
    want = {(h, k2): [k2] for h in range(2) for k2 in range(2)}
    assert block_a == want and block_b == want
    # -- opsel picks the byte of the scale register (the probe uses the same opsel for both operands)
    packed = torch.from_numpy(np.full((64,), 127 | (128 << 8) | (129 << 16) | (130 << 24), dtype=np.uint32).view(np.int32))
    unit = torch.from_numpy(np.full((64,), 0x7f7f7f7f, dtype=np.uint32).view(np.int32))
    for op in range(4):
        assert mat(run(ones(), ones(), packed, unit, op)).unique().tolist() == [64.0 * 2 ** op]
        assert mat(run(ones(), ones(), unit, packed, op)).unique().tolist() == [64.0 * 2 ** op]


# ------------------------------------------------------------------------------------------------ 2. the V dequantisation
@pytest.mark.parametrize("e", [-127, -20, 0, 7, 100])
def test_dequantisation_of_every_byte(yv, e):
    """Every e4m3 byte at the block exponent e through the conversion of the stash step (yv_attention_fp8_dequant runs the device
    function the kernel calls) against the decode of mx_reference, rounded once to bf16: exact wherever byte * 2^e is a bf16 number
    (4 significant bits: every case but the values below 2^-133 at e = -127, which round to a bf16 denormal or to zero)."""
    q = torch.arange(256, dtype=torch.uint8)
    got = yv.attention_fp8_dequant(q.to(DEV), e + 127)
    torch.cuda.synchronize()
    got = got.cpu()
    want = ref.to_bf16(mxr.dequant(q.view(1, 256), torch.full((1, 8), e + 127, dtype=torch.uint8)).numpy()).view(256)
    nan = torch.isnan(want)
    assert nan.nonzero().flatten().tolist() == [0x7f, 0xff]
    bad = ((got.view(torch.int16) != want.view(torch.int16)) & ~nan) | (nan & ~torch.isnan(got))
    print(f"e = {e}: {int(bad.sum())} of 256 bytes differ", [(hex(i), float(got[i]), float(want[i])) for i in bad.nonzero().flatten().tolist()][:8])
    assert not bool(bad.any())


# ------------------------------------------------------------------------------------------------ 3. exact scores
CODE = torch.tensor([0xC0, 0xB8, 0x00, 0x38, 0x40], dtype=torch.uint8)          # -2, -1, 0, 1, 2 in e4m3
SCALE = 2.0 ** -5


@functools.lru_cache(maxsize=None)
def exact_case(R, N, H):
    """An MXFP8 qkv operand whose scores are exact in f32 in any order (Q / K small integers at block exponents -1 .. 1; V random
    finite bytes at exponents -3 .. 3), its dequantised bf16 copy, and the outputs of yv_attention_long on that copy: bf16 rows,
    MX bytes and scale bytes."""
    import yvhip as yv
    rows, D = R * N, 64 * H
    g = torch.Generator().manual_seed(R * 100000 + N * 100 + H)
    q = torch.empty(rows, 3 * D, dtype=torch.uint8)
    q[:, :2 * D] = CODE[torch.randint(0, 5, (rows, 2 * D), generator=g)]
    v = torch.randint(0, 256, (rows, D), generator=g).to(torch.uint8)
    q[:, 2 * D:] = torch.where((v & 0x7f) == 0x7f, v - 1, v)                    # no NaN
    s = torch.empty(rows, 6 * H, dtype=torch.uint8)
    s[:, :4 * H] = torch.randint(126, 129, (rows, 4 * H), generator=g).to(torch.uint8)
    s[:, 4 * H:] = torch.randint(124, 131, (rows, 2 * H), generator=g).to(torch.uint8)
    deq = mxr.dequant(q, s)
    qkv = deq.to(torch.bfloat16)
    assert torch.equal(qkv.double(), deq)                                       # the copy is exact
    s_dev = device_scales(s, r128(rows))
    qkv_d = qkv.to(DEV)
    out = torch.zeros(rows, D, dtype=torch.bfloat16, device=DEV)
    oq = torch.zeros(rows, D, dtype=torch.uint8, device=DEV)
    osc = torch.zeros(D // 128, r128(rows), 4, dtype=torch.uint8, device=DEV)
    yv.attention_long(qkv_d, R, N, H, out, scale=SCALE, out_q=oq, out_scale=osc)
    torch.cuda.synchronize()
    return q.to(DEV), s_dev.to(DEV), out, oq, osc


def run_fp8(yv, q, s, R, N, H, r_dev=None, fill=0):
    rows, D = R * N, 64 * H
    out = torch.full((rows, D), fill, dtype=torch.bfloat16, device=DEV)
    oq = torch.full((rows, D), fill, dtype=torch.uint8, device=DEV)
    osc = torch.full((D // 128, r128(rows), 4), fill, dtype=torch.uint8, device=DEV)
    yv.attention_fp8(q, s, R, N, H, out, scale=SCALE, r_dev=r_dev, out_q=oq, out_scale=osc)
    torch.cuda.synchronize()
    return out, oq, osc


EXACT_SHAPES = [(2, 1, 2), (1, 31, 2), (1, 32, 2), (1, 33, 2), (1, 64, 2), (1, 65, 4), (2, 128, 2), (1, 129, 2), (2, 197, 4),
                (1, 257, 2), (1, 785, 2)]


@pytest.mark.parametrize("R,N,H", EXACT_SHAPES)
def test_exact_scores_give_the_bytes_of_attention_long(yv, R, N, H):
    q, s, want, want_q, want_s = exact_case(R, N, H)
    rows = R * N
    out, oq, osc = run_fp8(yv, q, s, R, N, H)
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) > 0
    assert torch.equal(out, want)
    assert torch.equal(oq, want_q) and torch.equal(osc[:, :rows], want_s[:, :rows])
    # the same from a wider row and a larger scale array (the strides are arguments)
    wide = torch.zeros(rows, q.shape[1] + 32, dtype=torch.uint8, device=DEV)
    wide[:, :q.shape[1]] = q
    s_big = torch.zeros(s.shape[0], s.shape[1] + 128, 4, dtype=torch.uint8, device=DEV)
    s_big[:, :s.shape[1]] = s
    out2 = torch.zeros_like(out)
    yv.attention_fp8(wide[:, :q.shape[1]], s_big, R, N, H, out2, scale=SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out2, want)


@pytest.mark.parametrize("R,N,H", [s for s in EXACT_SHAPES if s[0] == 2])
def test_crop_count_and_crop_independence(yv, R, N, H):
    q, s, want, want_q, want_s = exact_case(R, N, H)
    one = torch.tensor([1], dtype=torch.int32, device=DEV)
    out, oq, osc = run_fp8(yv, q, s, R, N, H, r_dev=one, fill=0x5B)
    assert torch.equal(out[:N], want[:N]) and torch.equal(oq[:N], want_q[:N]) and torch.equal(osc[:, :N], want_s[:, :N])
    sentinel = torch.full((1,), 0x5B, dtype=torch.bfloat16, device=DEV)
    assert bool((out[N:] == sentinel).all()) and bool((oq[N:] == 0x5B).all()) and bool((osc[:, N:] == 0x5B).all())
    # crop 0 alone (R = 1, its own scale array) equals crop 0 of the pair
    s_rows = mxr.scale_rows(s.cpu(), N)
    out1, oq1, osc1 = run_fp8(yv, q[:N].contiguous(), device_scales(s_rows, r128(N)).to(DEV), 1, N, H)
    assert torch.equal(out1, want[:N]) and torch.equal(oq1, want_q[:N]) and torch.equal(osc1[:, :N], want_s[:, :N])


# ------------------------------------------------------------------------------------------------ 4. random data
def bf16_step(m: float) -> float:
    return 2.0 ** (int(np.floor(np.log2(m))) - 7)


@pytest.mark.parametrize("R,N,H", [(2, 197, 2), (1, 257, 2), (1, 785, 2)])
def test_random_data_against_attention_long_and_f64(yv, R, N, H):
    """A random bf16 qkv quantised by yv_quant_mxfp8.  Against yv_attention_long on the dequantised copy: at most one bf16 step of
    the largest |output| (the contract between two forward kernels, DESIGN.md section 15.2: the two differ in the f32 summation
    order of a 64-term score).  Against the f64 statement: ||new - ref|| <= ||long - ref|| + ||new - long|| and every element of
    new - long is within that step, so rel-L2(new) <= rel-L2(long) + step sqrt(n) / ||ref||."""
    rows, D = R * N, 64 * H
    g = torch.Generator().manual_seed(R * 1000 + N)
    x = (torch.randn(rows, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    q, s = yv.quant_mxfp8(x)
    torch.cuda.synchronize()
    deq = mxr.dequant(q.cpu(), mxr.scale_rows(s.cpu(), rows))
    qkv = deq.to(torch.bfloat16)
    assert torch.equal(qkv.double(), deq)
    want = torch.zeros(rows, D, dtype=torch.bfloat16, device=DEV)
    yv.attention_long(qkv.to(DEV), R, N, H, want)
    got = torch.zeros_like(want)
    yv.attention_fp8(q, s, R, N, H, got)
    torch.cuda.synchronize()
    got, want = got.cpu().double(), want.cpu().double()
    f64 = torch.from_numpy(ref.attention_fp8(q.cpu(), s.cpu(), R, N, H, 0.125)["f64"])
    step = bf16_step(float(want.abs().max()))
    diff = float((got - want).abs().max())
    rel_new, rel_long = float((got - f64).norm() / f64.norm()), float((want - f64).norm() / f64.norm())
    print(f"({R}, {N}, {H}): max |fp8 - long| {diff:.3e} (one step {step:.3e}); rel-L2 vs f64: fp8 {rel_new:.3e}, long {rel_long:.3e}")
    assert diff <= step
    assert rel_new <= rel_long + step * (got.numel() ** 0.5) / float(f64.norm())


# ------------------------------------------------------------------------------------------------ 5. the producer
def test_qkv_producer_writes_linear_then_quant(yv):
    """linear_mxfp8_q(flags=0) for N = 3 D = 384 writes the bytes and scales of linear_mxfp8 followed by quant_mxfp8, and the
    attention's reading of the scale layout (attn_fp8_reference.decode) decodes them to the bf16 product."""
    g = torch.Generator().manual_seed(21)
    M, N, K = 2 * 197, 384, 128
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    aq, asc = yv.quant_mxfp8(a)
    wq, wsc = yv.quant_mxfp8(w)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    yv.linear_mxfp8(aq, asc, wq, wsc, bias, out)
    q_ref, s_ref = yv.quant_mxfp8(out)
    q = torch.zeros(M, N, dtype=torch.uint8, device=DEV)
    s = torch.zeros_like(s_ref)
    yv.linear_mxfp8_q(aq, asc, wq, wsc, bias, q, s, flags=0)
    torch.cuda.synchronize()
    assert torch.equal(q, q_ref) and torch.equal(s[:, :M], s_ref[:, :M])
    qb, sb, deq = mxr.emulate_quant(out.cpu().float())
    assert torch.equal(q.cpu(), qb) and np.array_equal(ref.decode(q, s), deq.numpy())
    # head 1 of K: K step D / 128 = 1, bytes 2 and 3 of a row's dword
    assert torch.equal(s[1, :M, 2:4].cpu(), sb[:, 6:8])


# ------------------------------------------------------------------------------------------------ 6. the engine
def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def engine_case(name):
    from oracle import boxes as ob, vit as ov
    R = 3
    sd = ov.init_wrapper_state(name, seed=11)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    P = 8 if "8" in name.split("_")[1] else 16
    pm = torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), P)) for r in range(R)]).to(torch.bfloat16)
    return sd, pm, ov.vit_forward(sd, x, name)[:, :1000]


def run_engine(sd, name, pm, R=3, **kw):
    from yvhip import engines
    eng = engines.VitEngine(sd, name, 5, device=DEV, dtype="mxfp8", **kw)
    cap = R + 1                                          # r_dev shorter than the capacity
    buf = eng.patch_buffer(cap)
    buf[:pm.shape[0]] = pm.to(DEV)
    cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
    feats = eng.backbone(buf, cap, cnt)
    torch.cuda.synchronize()
    return eng, buf, cnt, feats[:R, :1000].cpu()


def hand_chain(yv, eng, patches, cap, count):
    """The unflagged mxfp8 engine's pass with qkv -> quant_mxfp8 -> attention_fp8 in place of its attention."""
    D, N, H, tok = eng.D, eng.N, eng.H, eng.tok
    b = eng._buffers(cap, slot=1)
    x, qkv, hq, hs, gq, gs = b["x"], b["qkv"], b["q"], b["qs"], b["gq"], b["gs"]
    rows = cap * N
    yv.cls_rows(eng.cls, eng.pos, cap, tok, D, x)
    yv.linear(patches, eng.w_pe, eng.b_pe, x, flags=yv.EPI_OUT_F32 | yv.EPI_POSEMB, pos=eng.pos, tok=tok, m_dev=count, m_mul=tok)
    for blk in eng.blocks:
        yv.layernorm_mxfp8(x, blk["n1w"], blk["n1b"], hq, hs, rows, D, D, count_dev=count, rows_per_count=N)
        yv.linear_mxfp8(hq, hs, blk["wqkv_q"], blk["wqkv_s"], blk["bqkv"], qkv, m_dev=count, m_mul=N)
        q8, s8 = yv.quant_mxfp8(qkv)
        yv.attention_fp8(q8, s8, cap, N, H, r_dev=count, out_q=hq, out_scale=hs)
        yv.linear_mxfp8(hq, hs, blk["wproj_q"], blk["wproj_s"], blk["bproj"], x, flags=yv.EPI_RES_F32, m_dev=count, m_mul=N)
        yv.layernorm_mxfp8(x, blk["n2w"], blk["n2b"], hq, hs, rows, D, D, count_dev=count, rows_per_count=N)
        yv.linear_mxfp8_q(hq, hs, blk["wfc1_q"], blk["wfc1_s"], blk["bfc1"], gq, gs, flags=yv.EPI_GELU, m_dev=count, m_mul=N)
        yv.linear_mxfp8(gq, gs, blk["wfc2_q"], blk["wfc2_s"], blk["bfc2"], x, flags=yv.EPI_RES_F32, m_dev=count, m_mul=N)
    yv.layernorm(x, eng.nw, eng.nb, b["c"], cap, D, N * D, D, count_dev=count, rows_per_count=1)
    yv.linear(b["c"], eng.w_head, eng.b_head, b["feats"], flags=yv.EPI_OUT_F32, m_dev=count, m_mul=1)
    torch.cuda.synchronize()
    return b["feats"]


@pytest.mark.parametrize("name", ["vit_tiny_test", "vit_tiny8_test"])
def test_engine_equals_the_hand_run_chain_and_tracks_the_oracle(yv, name):
    """Bit for bit the unflagged engine's pieces with qkv -> quant_mxfp8 -> attention_fp8; against the fp32 oracle the flagged
    engine's rel-L2 within 1.5 x the unflagged mxfp8 engine's on the same weights and crops (a block goes from four quantised GEMM
    operands to seven independent e4m3 roundings of comparable size: sqrt(7 / 4) = 1.32, plus room for a small sample)."""
    sd, pm, oracle = engine_case(name)
    base, buf, cnt, f_base = run_engine(sd, name, pm)
    flagged, _, _, f_fp8 = run_engine(sd, name, pm, fp8_attn=True)
    assert flagged.fp8_attn and not base.fp8_attn and "qkv" not in flagged._buffers(4)
    chain = hand_chain(yv, base, buf, 4, cnt)[:3, :1000].cpu()
    assert torch.equal(f_fp8, chain)
    assert not torch.equal(f_fp8, f_base)
    e_fp8, e_base = rel_l2(f_fp8, oracle), rel_l2(f_base, oracle)
    print(f"{name}: rel-L2 to the fp32 oracle: fp8_attn {e_fp8:.4e}, mxfp8 {e_base:.4e}, ratio {e_fp8 / e_base:.3f}")
    assert e_fp8 <= 1.5 * e_base
    # the flag together with mid_gemm (another K order in the block-scaled GEMMs): the same rule against that engine
    _, _, _, f_mid8 = run_engine(sd, name, pm, fp8_attn=True, mid_gemm=True)
    _, _, _, f_mid = run_engine(sd, name, pm, mid_gemm=True)
    print(f"{name}, mid_gemm: fp8_attn {rel_l2(f_mid8, oracle):.4e}, mxfp8 {rel_l2(f_mid, oracle):.4e}")
    assert rel_l2(f_mid8, oracle) <= 1.5 * rel_l2(f_mid, oracle)


@pytest.mark.parametrize("name", ["vit_base_patch16_224", "vit_base_patch8_224"])
def test_engine_against_the_bf16_engine_is_reported(name):
    """rel-L2, minimum per-crop cosine and arg-max agreement of the backbone logits against the bf16 engine at 8 crops, flag off
    and on (printed; DESIGN.md section 40 records them against the project's bounds for an mxfp8 engine, 0.12 and 0.99)."""
    from yvhip import engines
    sd = engines.init_vit_wrapper_state(name, 5, seed=4)
    R = 8
    g = torch.Generator().manual_seed(2)
    e16 = engines.VitEngine(sd, name, 5, device=DEV)
    patches = (torch.rand(R * e16.tok, 3 * e16.P * e16.P, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
    want = e16.backbone(patches, R, cnt)[:, :1000].cpu().double()
    del e16
    for flag in (False, True):
        eng = engines.VitEngine(sd, name, 5, device=DEV, dtype="mxfp8", fp8_attn=flag)
        got = eng.backbone(patches, R, cnt)[:, :1000].cpu().double()
        del eng
        assert bool(torch.isfinite(got).all())
        cos = torch.nn.functional.cosine_similarity(got, want, dim=1)
        agree = float((got.argmax(1) == want.argmax(1)).float().mean())
        print(f"{name} fp8_attn={flag}: rel-L2 {rel_l2(got, want):.4f}, min cosine {float(cos.min()):.4f}, arg-max agreement {agree:.3f}")
