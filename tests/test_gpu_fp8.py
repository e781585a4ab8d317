"""MXFP8 linears (BASELINE.json configs[4]: FP8 classifier GEMMs) against a torch emulation on the CPU: the quantiser
must reproduce the emulated bytes and scales exactly; the block-scaled MFMA GEMM must equal the fp64 product of the
DEQUANTISED operands up to fp32 accumulation (products of two e4m3 values are exact in fp32)."""
import math

import pytest
import torch
import torch.nn.functional as F

from mx_reference import assert_edge_blocks, edge_rows, emulate_quant, scale_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def test_mx_mfma_layout(yv):
    """Executable statement of the v_mfma_scale_f32_16x16x128_f8f6f4 operand layout the GEMM relies on (measured, the
    image carries no ISA document): lane (row r, group g) holds K 16g..16g+15 and 64+16g..64+16g+15; the scale of the
    32-block j of row r is byte `opsel` of the scale register of lane (r, group j)."""
    ONE = 0x38
    def run(a, b, sa, sb, opsel=0):
        d = torch.zeros(64, 4, device=DEV)
        yv.check(yv.lib.yv_mx_probe(a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(), opsel, d.data_ptr(), None), "probe")
        torch.cuda.synchronize()
        return d.cpu()
    ones = lambda: torch.full((64, 32), ONE, dtype=torch.uint8, device=DEV)
    zeros = lambda: torch.zeros((64, 32), dtype=torch.uint8, device=DEV)
    s127 = lambda: torch.full((64,), 127, dtype=torch.int32, device=DEV)
    assert run(ones(), ones(), s127(), s127()).unique().tolist() == [128.0]
    row = 5
    for g in range(4):
        for half in range(2):
            a = zeros(); a[g * 16 + row, half * 16:(half + 1) * 16] = ONE          # 16 K elements of row 5
            block = (16 * g + 64 * half) // 32                                     # the MX block they belong to
            for j in range(4):
                sa = s127(); sa[j * 16 + row] = 128                                 # double the scale of block j
                d = run(a, ones(), sa, s127())
                exp = 32.0 if j == block else 16.0
                assert d[(row >> 2) * 16:(row >> 2) * 16 + 16, row & 3].unique().tolist() == [exp], (g, half, j)
    import numpy as np
    packed = torch.from_numpy(np.full((64,), 127 | (128 << 8) | (129 << 16) | (130 << 24), dtype=np.uint32).view(np.int32)).to(DEV)
    unit = torch.from_numpy(np.full((64,), 0x7f7f7f7f, dtype=np.uint32).view(np.int32)).to(DEV)     # 2^0 in every byte
    for op in range(4):                                      # the probe uses the same opsel for both scale operands
        assert run(ones(), ones(), packed, unit, op).unique().tolist() == [128.0 * 2 ** op]


@pytest.mark.parametrize("rows,K", [(64, 128), (197, 1024), (1000, 768), (130, 384)])
def test_quant_mxfp8_matches_emulation(yv, rows, K):
    g = torch.Generator().manual_seed(rows + K)
    x = (torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 2)).to(torch.bfloat16)
    x[3, :32] = 0                                            # an all-zero block
    x[5, 32:64] = 448.0                                      # exactly the format maximum
    x[6, 64:96] = 2.0 ** -20
    qb, sb, _ = emulate_quant(x.float())
    q, s = yv.quant_mxfp8(x.to(DEV))
    torch.cuda.synchronize()
    kb = K // 32                                              # device layout (K/128, rows_pad, 4) -> (rows, K/32)
    s_rows = s.cpu()[:, :rows].permute(1, 0, 2).reshape(rows, kb)
    assert torch.equal(s_rows, sb)
    assert torch.equal(q.cpu(), qb)


@pytest.mark.parametrize("M,N,K,kind", [(256, 256, 256, "f32"), (1000, 384, 1024, "f32"), (197 * 4, 1024, 1024, "bf16_bias"),
                                        (640, 512, 4096, "gelu"), (130, 128, 128, "res"),
                                        # persistent free-running MX kernel (gemm_p9_kernel<..., MX>: M >= 2048, N % 256 == 0, >= 192 tiles)
                                        (6304 + 37, 3072, 1024, "gelu"), (12608, 1024, 1024, "res"), (5000, 4096, 256, "f32"),
                                        (6304, 2304, 768, "bf16_bias"), (9999, 1024, 2048, "res")])
def test_linear_mxfp8_matches_dequantised_product(yv, M, N, K, kind):
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    _, _, ad = emulate_quant(a.float())
    _, _, wd = emulate_quant(w.float())
    aq, asc = yv.quant_mxfp8(a.to(DEV))
    wq, wsc = yv.quant_mxfp8(w.to(DEV))
    ref = ad @ wd.t()
    if kind == "f32":
        out = torch.zeros(M, N, device=DEV)
        yv.linear_mxfp8(aq, asc, wq, wsc, None, out, flags=yv.EPI_OUT_F32)
        torch.cuda.synchronize()
        assert torch.allclose(out.cpu().double(), ref, rtol=2e-5, atol=2e-5 * float(ref.abs().max()))
    elif kind == "res":
        x = torch.randn(M, N, generator=g)
        out = x.clone().to(DEV)
        yv.linear_mxfp8(aq, asc, wq, wsc, bias.to(DEV), out, flags=yv.EPI_RES_F32)
        torch.cuda.synchronize()
        exp = x.double() + ref + bias.double()
        assert torch.allclose(out.cpu().double(), exp, rtol=2e-5, atol=2e-5 * float(exp.abs().max()))
    else:
        out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        yv.linear_mxfp8(aq, asc, wq, wsc, bias.to(DEV), out, flags=yv.EPI_GELU if kind == "gelu" else 0)
        torch.cuda.synchronize()
        exp = (ref + bias.double()).float()
        exp = F.gelu(exp) if kind == "gelu" else exp
        err = float((out.cpu().float() - exp).norm() / exp.norm())
        assert err < 4e-3, err                                # bf16 output rounding
    # and the quantisation itself is a small perturbation of the bf16 product (MX blocks of 32, e4m3)
    full = a.double() @ w.double().t()
    assert float((ref - full).norm() / full.norm()) < 5e-2


def test_vit_engine_mxfp8_tracks_bf16(yv):
    """VitEngine(dtype="mxfp8") (block linears on the block-scaled MFMA, activations quantised in front of each GEMM)
    against the bf16 engine on the same weights and crops: backbone logits rel-L2 <= 0.12 and per-crop cosine >= 0.99
    (the arg-max of 1000 near-tied random-init logits agrees for 75 % of the crops and is only reported).  e4m3 has 3 mantissa bits (each quantised operand carries ~3 % element noise, ~0.5 %
    per 768-long dot product); 48 quantised GEMMs through a random-init network measured 8.4 % / see the printed line."""
    from yvhip import engines
    name = "vit_base_patch16_224"
    sd = engines.init_vit_wrapper_state(name, 5, seed=4)
    e16 = engines.VitEngine(sd, name, 5, device=DEV)
    e8 = engines.VitEngine(sd, name, 5, device=DEV, dtype="mxfp8")
    R = 24
    g = torch.Generator().manual_seed(2)
    patches = (torch.rand(R * e16.tok, 768, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
    f16 = e16.backbone(patches, R, cnt).clone()
    f8 = e8.backbone(patches, R, cnt).clone()
    torch.cuda.synchronize()
    a, b = f8[:, :1000].cpu().double(), f16[:, :1000].cpu().double()
    err = float((a - b).norm() / b.norm())
    agree = float((a.argmax(1) == b.argmax(1)).float().mean())
    print(f"mxfp8 vs bf16 backbone logits: rel-L2 {err:.4f}, arg-max agreement {agree:.3f}")
    cos = torch.nn.functional.cosine_similarity(a, b, dim=1)
    assert err < 0.12, err
    assert float(cos.min()) > 0.99, float(cos.min())
    assert agree >= 0.5, agree             # 1000 near-tied random-init logits: the arg-max is a noisy statistic here (measured 0.75)


def test_layernorm_mxfp8_equals_layernorm_then_quant(yv):
    """The fused LayerNorm -> MXFP8 kernel keeps the bf16 rounding of the two-kernel path, so bytes and scales must be
    identical to yv_layernorm followed by yv_quant_mxfp8 (device-side dynamic row count included)."""
    g = torch.Generator().manual_seed(6)
    rows, D = 394, 1024
    x = (torch.randn(rows, D, generator=g) * 3 + 0.5).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV); beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    cnt = torch.tensor([2], dtype=torch.int32, device=DEV)                      # 2 x 150 = 300 live rows
    h = torch.zeros(rows, D, dtype=torch.bfloat16, device=DEV)
    yv.layernorm(x, gamma, beta, h, rows, D, D, D, count_dev=cnt, rows_per_count=150)
    q_ref, s_ref = yv.quant_mxfp8(h)
    q = torch.zeros(rows, D, dtype=torch.uint8, device=DEV)
    s = torch.zeros_like(s_ref)
    yv.layernorm_mxfp8(x, gamma, beta, q, s, rows, D, D, count_dev=cnt, rows_per_count=150)
    torch.cuda.synchronize()
    assert torch.equal(q[:300], q_ref[:300]) and torch.equal(s[:, :300], s_ref[:, :300])
    assert float(q[300:].float().abs().sum()) == 0                              # rows past the count stay untouched


def test_linear_mxfp8_q_equals_linear_then_quant(yv):
    """fc1 -> fc2 hand-off: the GEMM epilogue that emits MXFP8 directly must equal the bf16-output GEMM followed by
    yv_quant_mxfp8, byte for byte (ragged M, device-side row count)."""
    g = torch.Generator().manual_seed(12)
    M, N, K = 330, 512, 256
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    aq, asc = yv.quant_mxfp8(a)
    wq, wsc = yv.quant_mxfp8(w)
    cnt = torch.tensor([3], dtype=torch.int32, device=DEV)                      # 3 x 100 live rows
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    yv.linear_mxfp8(aq, asc, wq, wsc, bias, out, flags=yv.EPI_GELU, m_dev=cnt, m_mul=100)
    q_ref, s_ref = yv.quant_mxfp8(out)
    q = torch.zeros(M, N, dtype=torch.uint8, device=DEV)
    s = torch.zeros_like(s_ref)
    yv.linear_mxfp8_q(aq, asc, wq, wsc, bias, q, s, flags=yv.EPI_GELU, m_dev=cnt, m_mul=100)
    torch.cuda.synchronize()
    assert torch.equal(q[:300], q_ref[:300]) and torch.equal(s[:, :300], s_ref[:, :300])
    assert float(q[300:].float().abs().sum()) == 0


def test_linear_mxfp8_q_persistent_equals_linear_then_quant(yv):
    """The same hand-off on the persistent MX kernel (ViT-L fc1 shape at 32 crops): byte-identical to the bf16-output GEMM of the
    same kernel followed by yv_quant_mxfp8, and to the 128 x 128 kernel's image (linear_p8 = 0)."""
    g = torch.Generator().manual_seed(13)
    M, N, K = 6304 + 19, 4096, 1024
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    aq, asc = yv.quant_mxfp8(a)
    wq, wsc = yv.quant_mxfp8(w)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    yv.linear_mxfp8(aq, asc, wq, wsc, bias, out, flags=yv.EPI_GELU)
    q_ref, s_ref = yv.quant_mxfp8(out)
    q = torch.zeros(M, N, dtype=torch.uint8, device=DEV)
    s = torch.zeros_like(s_ref)
    yv.linear_mxfp8_q(aq, asc, wq, wsc, bias, q, s, flags=yv.EPI_GELU)
    torch.cuda.synchronize()
    assert torch.equal(q, q_ref) and torch.equal(s[:, :M], s_ref[:, :M])
    try:
        yv.set_option("linear_p8", 0)
        out0 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        yv.linear_mxfp8(aq, asc, wq, wsc, bias, out0, flags=yv.EPI_GELU)
        torch.cuda.synchronize()
        assert torch.equal(out0, out)
    finally:
        yv.set_option("linear_p8", 3)


def test_pipeline_with_mxfp8_classifier(yv):
    """The whole detect -> crop -> classify pipeline with an MXFP8 classifier: the pipelined two-stream / split schedule
    gives bitwise the single-stream results (per-slot operand buffers, device-side crop count)."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline, PipelinedRunner
    name, S, B = "vit_tiny_test", 128, 4
    vit = engines.VitEngine(engines.init_vit_wrapper_state(name, 5, 4), name, 5, device=DEV, dtype="mxfp8")
    pipe = DetectClassifyPipeline(engines.YoloEngine(engines.init_yolo_state("n", 5, 3, 4.0), "n", 5, S, DEV), [vit],
                                  max_crops_per_image=3)
    g = torch.Generator().manual_seed(41)
    batches = [torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(4)]
    keys = ("crop_list", "crop_total", "cls_logits", "cls_label")
    ref = []
    for im in batches:
        o = pipe(im)
        torch.cuda.synchronize()
        ref.append({k: o[k].clone() for k in keys})
    assert any(int(r["crop_total"][0]) > 0 for r in ref)
    for split in (False, True):
        runner = PipelinedRunner(pipe, split_classifier=split)
        outs = [runner.submit(im) for im in batches]
        runner.sync()
        for o, r in zip(outs, ref):
            for k in keys:
                assert torch.equal(o[k], r[k]), (split, k)


@pytest.mark.parametrize("R,N,H", [(3, 197, 12), (2, 50, 2), (1, 785, 4)])
def test_attention_mxfp8_equals_attention_then_quant(yv, R, N, H):
    """Attention whose epilogue emits the MXFP8 operand of the proj GEMM: identical bytes and scales to yv_attention
    followed by yv_quant_mxfp8 (single-tile and online-softmax kernels, device-side crop count)."""
    g = torch.Generator().manual_seed(R * 1000 + N + H)
    D = H * 64
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    cnt = torch.tensor([max(R - 1, 1)], dtype=torch.int32, device=DEV)
    live = int(cnt[0]) * N
    o = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    yv.attention(qkv, R, N, H, o, r_dev=cnt)
    q_ref, s_ref = yv.quant_mxfp8(o)
    q = torch.zeros(R * N, D, dtype=torch.uint8, device=DEV)
    s = torch.zeros_like(s_ref)
    yv.attention_mxfp8(qkv, R, N, H, q, s, r_dev=cnt)
    torch.cuda.synchronize()
    assert torch.equal(q[:live], q_ref[:live]) and torch.equal(s[:, :live], s_ref[:, :live])
    assert float(q[live:].float().abs().sum()) == 0


# ---- edge blocks at the fused producers -------------------------------------------------------------------------------------
# Every fused producer is run on operands for which its bf16 operation is exactly the identity, so the expected bytes are the
# CPU reference (mx_reference) of a planted tensor that holds the blocks where the exponent rule's branches decide the byte: all
# zero, amax +-448 * 2^k (k = -3, 0, 5), amax 2^-20, amax 8 among smaller values (mx_reference.edge_rows).

@pytest.mark.parametrize("M,N,inst", [(130, 128, 0), (7880, 1024, 1)])
def test_linear_mxfp8_q_edge_blocks(yv, M, N, inst):
    """Linear -> MXFP8 with W = identity, zero bias, no activation and A the dequantised image of the planted tensor: every output is
    one exact product of a value that is exact in e4m3 and in bf16, so the image is mx_reference of A.  Once on the 128 x 128
    kernel's epilogue, once on the persistent kernel's (N = K = 1024 reaches it from 7521 rows on; the 7880 rows repeat 394 planted ones)."""
    assert yv.linear_mxfp8_instance(M, N, N) == inst
    base = edge_rows(min(M, 394), N, seed=M, exact=True)
    assert_edge_blocks(base)
    qb, sb, _ = emulate_quant(base)
    rep = M // base.shape[0]
    assert rep * base.shape[0] == M
    a = base.repeat(rep, 1).to(torch.bfloat16).to(DEV)
    aq, asc = yv.quant_mxfp8(a)
    wq, wsc = yv.quant_mxfp8(torch.eye(N, dtype=torch.bfloat16, device=DEV))
    q = torch.full((M, N), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full_like(asc, 0x5B)
    yv.linear_mxfp8_q(aq, asc, wq, wsc, torch.zeros(N, device=DEV), q, s)
    torch.cuda.synchronize()
    assert torch.equal(q.cpu(), qb.repeat(rep, 1))
    assert torch.equal(scale_rows(s.cpu(), M), sb.repeat(rep, 1))


@pytest.mark.parametrize("D", [128, 1024])
def test_layernorm_mxfp8_edge_blocks(yv, D):
    """LayerNorm -> MXFP8 with gamma = 0 and beta = one planted row: every live row is beta exactly.  The device-side row count
    cuts inside the last workgroup's four rows."""
    rows, per, live = 302, 99, 297                               # 297 = 74 * 4 + 1
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(rows, D, generator=g) * 3 + 0.5).to(DEV)
    cnt = torch.tensor([3], dtype=torch.int32, device=DEV)
    planted = edge_rows(-(-7 * 32 // D), D, seed=D)               # as many rows as hold the edge blocks once
    assert_edge_blocks(planted)
    qb, sb = emulate_quant(planted)[:2]
    for i in range(planted.shape[0]):
        q = torch.full((rows, D), 0xA5, dtype=torch.uint8, device=DEV)
        s = torch.full((D // 128, 512, 4), 0x5B, dtype=torch.uint8, device=DEV)
        yv.layernorm_mxfp8(x, torch.zeros(D, device=DEV), planted[i].to(DEV), q, s, rows, D, D, count_dev=cnt, rows_per_count=per)
        torch.cuda.synchronize()
        assert torch.equal(q[:live].cpu(), qb[i].expand(live, D))
        assert torch.equal(scale_rows(s.cpu(), live), sb[i].expand(live, D // 32))
        assert bool((q[live:] == 0xA5).all()) and bool((s[:, live:] == 0x5B).all())      # rows past the count stay untouched


def test_attention_mxfp8_edge_blocks_one_token(yv):
    """Attention -> MXFP8 at N = 1 (attention_pipe_kernel<1>): the softmax of one score is 1, the output is V exactly."""
    R, H = 5, 4
    D = H * 64
    g = torch.Generator().manual_seed(7)
    v = edge_rows(R, D, seed=3)
    assert_edge_blocks(v)
    qkv = (torch.randn(R, 3 * D, generator=g) * 0.7).to(torch.bfloat16)
    qkv[:, 2 * D:] = v.to(torch.bfloat16)
    qb, sb = emulate_quant(v)[:2]
    q = torch.full((R, D), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full((D // 128, 128, 4), 0x5B, dtype=torch.uint8, device=DEV)
    yv.attention_mxfp8(qkv.to(DEV), R, 1, H, q, s)
    torch.cuda.synchronize()
    assert torch.equal(q.cpu(), qb) and torch.equal(scale_rows(s.cpu(), R), sb)


def test_attention_mxfp8_zero_head(yv):
    """Attention -> MXFP8 at N = 785 (attention_kernel, online softmax): V of one head is zero, so that head's two blocks of every
    row are all-zero blocks - scale byte 0, zero bytes; the other heads equal attention followed by yv_quant_mxfp8."""
    R, N, H, zh = 1, 785, 4, 2
    D = H * 64
    g = torch.Generator().manual_seed(R * 1000 + N + H + 1)
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 0.7).to(torch.bfloat16)
    qkv[:, 2 * D + zh * 64:2 * D + (zh + 1) * 64] = 0
    qkv = qkv.to(DEV)
    o = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    yv.attention(qkv, R, N, H, o)
    q_ref, s_ref = yv.quant_mxfp8(o)
    q = torch.full((R * N, D), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full_like(s_ref, 0x5B)
    yv.attention_mxfp8(qkv, R, N, H, q, s)
    torch.cuda.synchronize()
    assert bool((q[:, zh * 64:(zh + 1) * 64] == 0).all())
    assert bool((scale_rows(s.cpu(), R * N)[:, 2 * zh:2 * zh + 2] == 0).all())
    assert torch.equal(q, q_ref) and torch.equal(s[:, :R * N], s_ref[:, :R * N])
