"""GPU checks of the fused residual + LayerNorm GEMM: yv_linear_res_ln on exact small-integer operands and on random ones,
the independence of a row's outputs from M / the device count / the grid, VitEngine(fused_ln=True) against the unfused engine and
the fp32 oracle, and the fused engine through PipelinedRunner.  The kernel has ONE tile height (64 rows) and one instance per
width, so there is no instance option to force (the issue's "tile variants" item has nothing to test)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import boxes as ob, vit as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BM = 64                                                # the kernel's tile height
EPS = 1e-6


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def bf(t):
    return t.to(torch.bfloat16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def ln64(x, gamma, beta):
    return F.layer_norm(x.double(), (x.shape[1],), gamma.double(), beta.double(), EPS)


def h_ratio(h, v):
    """Largest |h - v| / (2^-8 |v| + 1e-4): bf16 half-ulp of the fp64 value + f32 slack; <= 1 passes."""
    return float(((h.double() - v).abs() / (2.0 ** -8 * v.abs() + 1e-4)).max())


# ------------------------------------------------------------------------------------------------ 1. exact integers
NK = [(128, 128), (128, 512), (768, 768), (768, 3072), (768, 192), (1024, 1024), (1024, 4096)]
MS = sorted({1, 37, 197, 394, BM - 1, BM, BM + 1, 3 * BM + 5})
M_MAX = max(MS)
_REF = {}


def int_case(N, K):
    """Operands and references of one (N, K) for M_MAX rows, made once (a smaller M takes the first M rows)."""
    if (N, K) not in _REF:
        g = torch.Generator().manual_seed(N * 3 + K)
        a = torch.randint(-2, 3, (M_MAX, K), generator=g).float()
        w = torch.randint(-2, 3, (N, K), generator=g).float()
        bias = torch.randint(-8, 9, (N,), generator=g).float()
        x = torch.randint(-64, 65, (M_MAX, N), generator=g).float()
        gamma = 1 + 0.1 * torch.randn(N, generator=g)
        beta = 0.1 * torch.randn(N, generator=g)
        xn = x + a @ w.t() + bias                              # exact: every |sum| < 2^24
        assert float(xn.abs().max()) < 2 ** 24
        _REF[(N, K)] = dict(a=a, w=w, bias=bias, x=x, gamma=gamma, beta=beta, xn=xn, v=ln64(xn, gamma, beta))
    return _REF[(N, K)]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", NK)
def test_linear_res_ln_exact_integer(yv, N, K, M):
    """x must EQUAL x + a @ w.t() + bias (exact whatever the K order), h stays within 2^-8 |v| + 1e-4 of the fp64 LayerNorm v of
    that x; contiguous and with padded lda / ldx / ldh, with and without a device row count (rows past it and the padding keep
    their fill in both buffers), twice (bit-identical)."""
    c = int_case(N, K)
    wd, bd, gd, btd = bf(c["w"]).to(DEV), c["bias"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV)
    worst = 0.0
    for pa, px, ph in ((0, 0, 0), (8, 16, 24)):                # column padding of a / x / h rows, in elements
        abuf = torch.full((M, K + pa), 7.0, dtype=torch.bfloat16, device=DEV)
        abuf[:, :K] = bf(c["a"][:M]).to(DEV)
        for m_dev in (None, torch.tensor([M // 3], dtype=torch.int32, device=DEV)):
            rows = M if m_dev is None else M // 3
            outs = []
            for rep in range(2):
                xbuf = torch.full((M, N + px), -5.0, device=DEV)
                xbuf[:, :N] = c["x"][:M].to(DEV)
                hbuf = torch.full((M, N + ph), 3.0, dtype=torch.bfloat16, device=DEV)
                yv.linear_res_ln(abuf[:, :K], wd, bd, xbuf[:, :N], gd, btd, hbuf[:, :N], eps=EPS, m_dev=m_dev, m_mul=1)
                torch.cuda.synchronize()
                outs.append((xbuf.cpu(), hbuf.cpu().float()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # determinism
            xo, ho = outs[0]
            assert torch.equal(xo[:rows, :N], c["xn"][:rows])
            if rows:
                r = h_ratio(ho[:rows, :N], c["v"][:rows])
                worst = max(worst, r)
                assert r <= 1.0, (pa, rows, r)
            assert torch.equal(xo[rows:, :N], c["x"][rows:M])                                     # rows past the count: untouched
            assert torch.equal(ho[rows:, :N], torch.full((M - rows, N), 3.0))
            assert torch.equal(xo[:, N:], torch.full((M, px), -5.0))                              # padding between the rows
            assert torch.equal(ho[:, N:], torch.full((M, ph), 3.0))
    print(f"\nres_ln exact M={M} N={N} K={K}: largest h error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 2. random operands
@pytest.mark.parametrize("M,N,K", [(394, 768, 768), (394, 768, 3072), (130, 1024, 4096)])
def test_linear_res_ln_random(yv, M, N, K):
    """x no further from fp64 than twice the unfused yv_linear (YV_EPI_RES_F32) is, h within the bound of test 1 of the fp64
    LayerNorm of the kernel's own x - and, beyond what the bound asks, equal to yv_layernorm of that x bit for bit."""
    g = torch.Generator().manual_seed(M + N + K)
    a, w = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g))
    bias, x = torch.randn(N, generator=g), torch.randn(M, N, generator=g) * 3
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    ref = x.double() + a.double() @ w.double().t() + bias.double()
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    xu = x.to(DEV).clone()
    yv.linear(ad, wd, bd, xu, flags=yv.EPI_RES_F32)
    xf, hf = x.to(DEV).clone(), torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    yv.linear_res_ln(ad, wd, bd, xf, gamma.to(DEV), beta.to(DEV), hf, eps=EPS)
    hl = torch.zeros_like(hf)
    yv.layernorm(xf, gamma.to(DEV), beta.to(DEV), hl, M, N, N, N, eps=EPS)
    torch.cuda.synchronize()
    assert torch.equal(hl, hf)                 # the statistics are summed in yv_layernorm's order: its bits on the same x
    eu, ef = rel_l2(xu.cpu(), ref), rel_l2(xf.cpu(), ref)
    r = h_ratio(hf.cpu().float(), ln64(xf.cpu(), gamma, beta))
    print(f"\nres_ln random ({M},{N},{K}): x rel-L2 fused {ef:.3e} unfused {eu:.3e}; h error / bound {r:.3f}")
    assert ef <= max(2 * eu, 1e-6)
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("N,K", [(768, 768), (1024, 1024), (128, 512)])
def test_linear_res_ln_row_independence(yv, N, K):
    """Rows 0..196 of an M = 394 call equal an M = 197 call on the same rows bit for bit, and the M = 394 result does not depend on
    the grid (two workgroups walk the seven tiles)."""
    g = torch.Generator().manual_seed(N + K)
    M = 394
    a, w = bf(torch.randn(M, K, generator=g)).to(DEV), bf(torch.randn(N, K, generator=g)).to(DEV)
    bias, x = torch.randn(N, generator=g).to(DEV), (torch.randn(M, N, generator=g) * 3).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(N, generator=g)).to(DEV), (0.1 * torch.randn(N, generator=g)).to(DEV)

    def run(rows):
        xo, ho = x[:rows].clone(), torch.zeros(rows, N, dtype=torch.bfloat16, device=DEV)
        yv.linear_res_ln(a[:rows], w, bias, xo, gamma, beta, ho, eps=EPS)
        torch.cuda.synchronize()
        return xo.cpu(), ho.cpu().float()

    x394, h394 = run(394)
    x197, h197 = run(197)
    assert torch.equal(x394[:197], x197) and torch.equal(h394[:197], h197)
    assert not torch.equal(x394, x.cpu())
    prev = yv.get_option("linear_p8_cus")
    yv.set_option("linear_p8_cus", 2)
    try:
        x2, h2 = run(394)
    finally:
        yv.set_option("linear_p8_cus", prev)
    assert torch.equal(x2, x394) and torch.equal(h2, h394)


# ------------------------------------------------------------------------------------------------ 5. engine
@pytest.mark.parametrize("name,R", [("vit_tiny_test", 3), ("vit_tiny8_test", 2), ("vit_base_patch16_224", 2),
                                    ("vit_large_patch16_224", 1)])
def test_vit_engine_fused_ln(yv, monkeypatch, name, R):
    """VitEngine(fused_ln=True) against the unfused engine and the fp32 oracle, both cls_tail values, a spare slot and a device count
    below capacity: (a) the project's 2e-2 against the oracle, (b) closer to the unfused engine than that one is to the oracle,
    (c) labels on the `sure` rows, (d) rows past the count, (e) the LayerNorm launches that remain."""
    from yvhip import engines
    sd = ov.init_wrapper_state(name, seed=11)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    ref_feats = ov.vit_forward(sd, x, name)
    ref_logits = ov.wrapper_head(sd, ref_feats)
    margin = ref_logits.topk(2, 1).values
    sure = (margin[:, 0] - margin[:, 1]) > 0.05 * ref_logits.abs().max()
    calls = []
    real_ln = engines.layernorm
    monkeypatch.setattr(engines, "layernorm", lambda *a, **k: (calls.append(1), real_ln(*a, **k))[1])
    for tail in (True, False):
        res = {}
        for fused in (True, False):
            eng = engines.VitEngine(sd, name, 5, cls_tail=tail, fused_ln=fused)
            assert eng.fused_ln is fused
            pm = torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), eng.P)) for r in range(R)]).to(torch.bfloat16).to(DEV)
            cap = R + 1                                      # one spare slot: the device count leaves it untouched
            buf = eng.patch_buffer(cap)
            buf[:pm.shape[0]] = pm
            cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
            del calls[:]
            feats = eng.backbone(buf, cap, cnt)
            n_ln = len(calls)
            logits = torch.zeros(cap, 5, device=DEV); labels = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
            eng.head(feats, cap, logits, labels, count=cnt)
            torch.cuda.synchronize()
            assert n_ln == ((3 if tail else 2) if fused else 2 * eng.L + 1)                                   # (e)
            assert float(feats[:R, 1000:].abs().sum()) == 0
            assert int(labels[R]) == -1 and float(logits[R].abs().sum()) == 0                                 # (d)
            res[fused] = (feats[:R, :1000].cpu().clone(), logits[:R].cpu().clone(), labels[:R].cpu().clone())
            del eng
        (ff, fl, flab), (uf, ul, ulab) = res[True], res[False]
        figs = dict(fused_vs_oracle=(rel_l2(ff, ref_feats), rel_l2(fl, ref_logits)),
                    unfused_vs_oracle=(rel_l2(uf, ref_feats), rel_l2(ul, ref_logits)),
                    fused_vs_unfused=(rel_l2(ff, uf), rel_l2(fl, ul)))
        print(f"\n{name} R={R} cls_tail={tail} (feats, logits) rel-L2: " +
              ", ".join(f"{k} ({a:.3e}, {b:.3e})" for k, (a, b) in figs.items()))
        assert figs["fused_vs_oracle"][0] < 2e-2 and figs["fused_vs_oracle"][1] < 2e-2                        # (a)
        assert figs["fused_vs_unfused"][0] < figs["unfused_vs_oracle"][0]                                     # (b)
        assert figs["fused_vs_unfused"][1] < figs["unfused_vs_oracle"][1]
        assert flab[sure].tolist() == ref_logits.argmax(1)[sure].tolist()                                     # (c)
        assert flab[sure].tolist() == ulab[sure].tolist()


def test_vit_engine_fused_ln_switch(yv, monkeypatch):
    from yvhip import engines
    name = "vit_tiny_test"
    sd = engines.init_vit_wrapper_state(name, 5, 4)
    with pytest.raises(yv.YvError):                                                                           # (f)
        engines.VitEngine(sd, name, 5, dtype="mxfp8", fused_ln=True)
    monkeypatch.delenv("YV_VIT_FUSED_LN", raising=False)                                                      # (g)
    assert engines.VitEngine(sd, name, 5).fused_ln is False
    monkeypatch.setenv("YV_VIT_FUSED_LN", "1")
    assert engines.VitEngine(sd, name, 5).fused_ln is True
    assert engines.VitEngine(sd, name, 5, fused_ln=False).fused_ln is False
    assert engines.VitEngine(sd, name, 5, dtype="mxfp8").fused_ln is False         # the variable is the bf16 engine's
    monkeypatch.delenv("YV_VIT_FUSED_LN")
    assert engines.VitEngine(sd, name, 5).fused_ln is False


# ------------------------------------------------------------------------------------------------ 6. pipeline
def test_pipelined_runner_fused_ln_matches_single_stream():
    """The fused engine through PipelinedRunner(split_classifier=True) - half batches on two streams, a reduced CU budget -
    equals the fused engine single-stream bit for bit (toy size of test_pipelined_runner_matches_single_stream)."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline, PipelinedRunner
    name, S, B = "vit_tiny_test", 128, 4
    vit = engines.VitEngine(engines.init_vit_wrapper_state(name, 5, 4), name, 5, device=DEV, fused_ln=True)
    assert vit.fused_ln
    pipe = DetectClassifyPipeline(engines.YoloEngine(engines.init_yolo_state("n", 5, 3, 4.0), "n", 5, S, DEV), [vit],
                                  max_crops_per_image=3)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(5)]
    keys = ("det_count", "det_box", "det_score", "crop_list", "crop_total", "cls_logits", "cls_label")
    ref = []
    for im in batches:
        o = pipe(im)
        torch.cuda.synchronize()
        ref.append({k: o[k].clone() for k in keys})
    assert any(int(r["crop_total"].sum()) > 0 for r in ref)
    runner = PipelinedRunner(pipe, split_classifier=True)
    outs = [runner.submit(im) for im in batches]
    runner.sync()
    for o, r in zip(outs, ref):
        assert o["done"].query()
        for k in keys:
            assert torch.equal(o[k], r[k]), k
