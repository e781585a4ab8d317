"""GPU checks of the cls-row tail of the classifier's last block: the skinny-M linear route (exact small-integer operands),
yv_attention_cls against the fp32 formula and against row 0 of yv_attention, and VitEngine(cls_tail=True) against
VitEngine(cls_tail=False) and the fp32 oracle."""
import pytest
import torch
import torch.nn.functional as F

from oracle import boxes as ob, vit as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def bf(t):
    return t.to(torch.bfloat16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ skinny linear
SHAPES = [(M, N, K) for M in (1, 3, 64, 128, 130, 256) for N in (768, 1024, 3072) for K in (768, 3072, 1024)]


@pytest.mark.parametrize("kind", ["plain", "gelu", "res", "f32"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_skinny_linear_exact_integer(yv, M, N, K, kind):
    """Small-integer operands make every f32 sum exact (the scheme of test_linear_exact_integer): bias -> bf16, bias + f32
    residual read-modify-write and bias -> f32 must EQUAL the integer reference whatever the K slicing; GELU stays within the
    project's 3e-3.  Each case runs contiguous and with strided A rows / output rows, with and without the device-side row
    count (rows past it keep their contents), and twice (bit-identical)."""
    assert M <= yv.get_option("linear_skinny")                 # these shapes are the skinny route's
    g = torch.Generator().manual_seed(M * 7 + N + K)
    a = torch.randint(-2, 3, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    lin = a @ w.t() + bias                                     # exact: |sum| < 2^24
    x = torch.randint(-64, 65, (M, N), generator=g).float()
    flags = {"plain": 0, "gelu": yv.EPI_GELU, "res": yv.EPI_RES_F32, "f32": yv.EPI_OUT_F32}[kind]
    f32 = kind in ("res", "f32")
    for m_dev in (False, True):
        r = yv.linear_route(M, N, K, flags | yv.EPI_BIAS, m_dev=m_dev)
        assert (r.kernel, r.tile_rows, r.tile_cols, r.splitk) == (yv.LIN_SKINNY, 64, 16, 1)
    wd, bd = bf(w).to(DEV), bias.to(DEV)
    fill = 3.0

    def expect(got, rows):
        if kind == "res":
            assert torch.equal(got[:rows], (x + lin)[:rows])
        elif kind == "f32":
            assert torch.equal(got[:rows], lin[:rows])
        elif kind == "plain":
            assert torch.equal(got[:rows], bf(lin).float()[:rows])
        else:
            assert rel_l2(got[:rows], F.gelu(lin)[:rows]) < 3e-3
        if kind == "res":
            assert torch.equal(got[rows:], x[rows:])
        elif kind == "f32":
            assert torch.equal(got[rows:], x[rows:])
        else:
            assert torch.equal(got[rows:], torch.full((M - rows, N), fill))

    for sa, so in ((1, 1), (3, 2)):                            # row strides: sa * K for A, so * N for the output
        abuf = torch.full((M * sa, K), 7.0, dtype=torch.bfloat16, device=DEV)
        abuf[::sa] = bf(a).to(DEV)
        ad = abuf[::sa]
        for m_dev in (None, torch.tensor([M // 3], dtype=torch.int32, device=DEV)):
            rows = M if m_dev is None else min(M, M // 3)
            outs = []
            for rep in range(2):
                if f32:
                    obuf = torch.full((M * so, N), -5.0, device=DEV)
                    obuf[::so] = x.to(DEV)
                else:
                    obuf = torch.full((M * so, N), fill, dtype=torch.bfloat16, device=DEV)
                yv.linear(ad, wd, bd, obuf[::so], flags=flags, m_dev=m_dev, m_mul=1)
                torch.cuda.synchronize()
                outs.append(obuf.cpu().float())
            assert torch.equal(outs[0], outs[1])               # determinism
            expect(outs[0][::so], rows)
            if so > 1:                                         # the rows in between are untouched
                between = outs[0].view(M, so, N)[:, 1:]
                assert torch.equal(between, torch.full_like(between, -5.0 if f32 else fill))


def test_skinny_linear_residual_cls_stride(yv):
    """The tail's own form: residual read-modify-write on the cls rows of a (R * 197, 768) f32 stream (ldo = 197 * 768), A a compact
    (R, K) operand; every other row of the stream keeps its contents."""
    R, Ntok, D, K = 64, 197, 768, 3072
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-2, 3, (R, K), generator=g).float()
    w = torch.randint(-2, 3, (D, K), generator=g).float()
    bias = torch.randint(-8, 9, (D,), generator=g).float()
    x = torch.randint(-64, 65, (R * Ntok, D), generator=g).float()
    lin = a @ w.t() + bias
    xd = x.clone().to(DEV)
    cnt = torch.tensor([50], dtype=torch.int32, device=DEV)
    yv.linear(bf(a).to(DEV), bf(w).to(DEV), bias.to(DEV), xd[::Ntok], flags=yv.EPI_RES_F32, m_dev=cnt, m_mul=1)
    torch.cuda.synchronize()
    exp = x.clone()
    exp[::Ntok][:50] += lin[:50]
    assert torch.equal(xd.cpu(), exp)


def test_skinny_route_agrees_with_tiled_route(yv):
    """Same data through the 128 x 128 route (linear_skinny = 0): integers, so bit for bit."""
    M, N, K = 130, 1024, 768
    g = torch.Generator().manual_seed(4)
    a = bf(torch.randint(-2, 3, (M, K), generator=g).float()).to(DEV)
    w = bf(torch.randint(-2, 3, (N, K), generator=g).float()).to(DEV)
    bias = torch.randint(-8, 9, (N,), generator=g).float().to(DEV)
    o1 = torch.zeros(M, N, device=DEV); o2 = torch.zeros(M, N, device=DEV)
    assert yv.linear_route(M, N, K, yv.EPI_BIAS | yv.EPI_OUT_F32).kernel == yv.LIN_SKINNY
    yv.linear(a, w, bias, o1, flags=yv.EPI_OUT_F32)
    yv.set_option("linear_skinny", 0)
    try:
        r = yv.linear_route(M, N, K, yv.EPI_BIAS | yv.EPI_OUT_F32)
        assert (r.kernel, r.tile_rows, r.tile_cols) == (yv.LIN_DMA, 128, 128)
        yv.linear(a, w, bias, o2, flags=yv.EPI_OUT_F32)
    finally:
        yv.set_option("linear_skinny", 256)
    assert torch.equal(o1, o2)


# ------------------------------------------------------------------------------------------------ attention_cls
def _att_ref(qkv, R, N, H):
    t = qkv.float().view(R, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    att = ((t[0][:, :, :1] * 0.125) @ t[1].transpose(-2, -1)).softmax(-1)          # query 0 only
    return (att @ t[2]).transpose(1, 2).reshape(R, H * 64)


@pytest.mark.parametrize("R,N,H", [(3, 197, 12), (2, 5, 2), (2, 50, 2), (1, 256, 3), (2, 33, 1), (1, 64, 2),
                                   (2, 785, 3), (1, 257, 2), (1, 512, 1), (1, 1000, 2), (2, 197, 16)])
def test_attention_cls(yv, R, N, H):
    g = torch.Generator().manual_seed(R * 7 + N)
    D = H * 64
    qkv = bf(torch.randn(R * N, 3 * D, generator=g) * 1.5)
    ref = _att_ref(qkv, R, N, H)
    qd = qkv.to(DEV)
    q = qd[::N, :D].contiguous()
    out = torch.zeros(R, D, dtype=torch.bfloat16, device=DEV)
    yv.attention_cls(q, qd, R, N, H, out)
    got = out.cpu().float()
    print(f"\nattention_cls R={R} N={N} H={H}: rel-L2 vs fp32 {rel_l2(got, ref):.2e}")
    assert rel_l2(got, ref) < 8e-3
    assert torch.allclose(got, ref, atol=3e-2, rtol=2e-2)
    # row 0 of the full kernel on the same buffer
    full = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    yv.attention(qd, R, N, H, full)
    row0 = full[::N].cpu().float()
    print(f"attention_cls vs yv_attention row 0: rel-L2 {rel_l2(got, row0):.2e}")
    assert rel_l2(got, row0) < 8e-3
    assert torch.allclose(got, row0, atol=3e-2, rtol=2e-2)


def test_attention_cls_softmax_spike(yv):
    # one key dominates the cls query (forces a large max subtraction)
    R, N, H = 1, 197, 1
    g = torch.Generator().manual_seed(5)
    qkv = bf(torch.randn(N, 192, generator=g))
    qkv[0, :64] = 8.0; qkv[100, 64:128] = 8.0
    ref = _att_ref(qkv, R, N, H)
    qd = qkv.to(DEV)
    out = torch.zeros(1, 64, dtype=torch.bfloat16, device=DEV)
    yv.attention_cls(qd[:1, :64].contiguous(), qd, R, N, H, out)
    assert torch.allclose(out.cpu().float(), ref, atol=3e-2, rtol=2e-2)
    assert torch.allclose(out.cpu().float()[0], qkv.float()[100, 128:], atol=2e-2)


def test_attention_cls_device_count(yv):
    R, N, H = 3, 197, 2
    g = torch.Generator().manual_seed(8)
    D = H * 64
    qkv = bf(torch.randn(R * N, 3 * D, generator=g))
    ref = _att_ref(qkv, R, N, H)
    qd = qkv.to(DEV)
    out = torch.full((R, D), 3.0, dtype=torch.bfloat16, device=DEV)
    cnt = torch.tensor([1], dtype=torch.int32, device=DEV)
    yv.attention_cls(qd[::N, :D].contiguous(), qd, R, N, H, out, r_dev=cnt)
    got = out.cpu().float()
    assert rel_l2(got[:1], ref[:1]) < 8e-3
    assert torch.equal(got[1:], torch.full((R - 1, D), 3.0))           # rows past the count stay untouched


# ------------------------------------------------------------------------------------------------ engine parity
@pytest.mark.parametrize("name,R", [("vit_tiny_test", 3), ("vit_base_patch16_224", 2), ("vit_tiny8_test", 2),
                                    ("vit_large_patch16_224", 1)])
def test_vit_engine_cls_tail_vs_full(name, R):
    """VitEngine(cls_tail=True) against VitEngine(cls_tail=False) on the same weights and crops (spare slot and device count of
    test_vit_engine_vs_oracle).  Same mathematics; they differ in the f32 summation order of five small products and the bf16
    re-roundings that follow.  Required: (a) the pruned engine meets the project's 2e-2 against the fp32 oracle on feats and
    logits, (b) rel-L2(pruned, full) < rel-L2(full, oracle) on both - the two builds are closer to each other than bf16
    arithmetic is to fp32, (c) labels agree on the `sure` rows."""
    from yvhip import engines
    sd = ov.init_wrapper_state(name, seed=11)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    ref_feats = ov.vit_forward(sd, x, name)
    ref_logits = ov.wrapper_head(sd, ref_feats)
    res = {}
    for tail in (True, False):
        eng = engines.VitEngine(sd, name, 5, cls_tail=tail)
        assert eng.cls_tail is tail
        pm = torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), eng.P)) for r in range(R)]).to(torch.bfloat16).to(DEV)
        cap = R + 1                                      # one spare slot: dynamic count leaves it untouched
        buf = eng.patch_buffer(cap)
        buf[:pm.shape[0]] = pm
        cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
        feats = eng.backbone(buf, cap, cnt)
        logits = torch.zeros(cap, 5, device=DEV); labels = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
        eng.head(feats, cap, logits, labels, count=cnt)
        torch.cuda.synchronize()
        assert float(feats[:R, 1000:].abs().sum()) == 0
        assert int(labels[R]) == -1 and float(logits[R].abs().sum()) == 0
        res[tail] = (feats[:R, :1000].cpu().clone(), logits[:R].cpu().clone(), labels[:R].cpu().clone())
        del eng
    (pf, pl, plab), (ff, fl, flab) = res[True], res[False]
    figs = dict(pruned_vs_oracle=(rel_l2(pf, ref_feats), rel_l2(pl, ref_logits)),
                full_vs_oracle=(rel_l2(ff, ref_feats), rel_l2(fl, ref_logits)),
                pruned_vs_full=(rel_l2(pf, ff), rel_l2(pl, fl)))
    print(f"\n{name} R={R} (feats, logits) rel-L2: " + ", ".join(f"{k} ({a:.3e}, {b:.3e})" for k, (a, b) in figs.items()))
    assert figs["pruned_vs_oracle"][0] < 2e-2 and figs["pruned_vs_oracle"][1] < 2e-2                      # (a)
    assert figs["pruned_vs_full"][0] < figs["full_vs_oracle"][0]                                          # (b)
    assert figs["pruned_vs_full"][1] < figs["full_vs_oracle"][1]
    margin = ref_logits.topk(2, 1).values
    sure = (margin[:, 0] - margin[:, 1]) > 0.05 * ref_logits.abs().max()
    assert plab[sure].tolist() == ref_logits.argmax(1)[sure].tolist()                                     # (c)
    assert plab[sure].tolist() == flab[sure].tolist()
