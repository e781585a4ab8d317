"""GPU checks of the fused LayerNorm + linear (gemm_mid_ln_kernel, yv_linear_ln, option "linear_ln_mid").
The contract: given the same x, linear_ln's output has the bits of layernorm followed by linear on the mid-M route, for every
accepted shape and flag set, on random data; nothing but the result is written; the pair route is the pair.  Then the engine
(VitEngine(ln_gemm=True)) and the request pipeline on top of it."""
import contextlib

import pytest
import torch

from oracle import boxes as ob
from oracle import vit as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 3152                              # engines.MID_GEMM_ROWS: what an ln_gemm pass sets "linear_ln_mid" to
NC = 5


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@contextlib.contextmanager
def options(yv, **kw):
    old = {k: yv.get_option(k) for k in kw}
    for k, v in kw.items():
        yv.set_option(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def every_shape(yv):
    """Both steps on and both fill rules raised: the pair's linear on gemm_mid_kernel, linear_ln on gemm_mid_ln_kernel."""
    return options(yv, linear_mid=ROWS, linear_mid_fill=1 << 20, linear_ln_mid=ROWS, linear_ln_fill=1 << 20)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _data(M, N, K, seed):
    """x: N(0, 1) x 3 plus a per-row offset up to +-50, row 5 constant (variance 0); gamma of both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 3 + (torch.rand(M, 1, generator=g) * 100 - 50)
    x[5] = 7.25
    gamma = torch.randn(K, generator=g)
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    beta = torch.randn(K, generator=g) * 0.5
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    return x, gamma, beta, w, bias


FLAG_SETS = {"plain": lambda yv: 0, "bias": lambda yv: yv.EPI_BIAS, "gelu": lambda yv: yv.EPI_BIAS | yv.EPI_GELU,
             "f32": lambda yv: yv.EPI_BIAS | yv.EPI_OUT_F32}
# K: 64 one K step (half 1 adds zeros), 128 one step per half, 192 an odd count (half 1 idles on the last trip), 768, 1024 four
# float4 chunks per lane (the LN_MAXC bound).  M: 257 one live row in the last tile, 320 whole tiles, 394 with a device count
# ending mid-tile.  N: 64 one column tile, 192 three, 128 two.
CASES = [(257, 64, 64), (257, 192, 128), (320, 128, 192), (320, 192, 768), (257, 64, 1024), (394, 192, 768), (394, 128, 1024)]
FILL = 3.0


def _run(yv, M, N, K, kind, fused, seed):
    """One call on strided operands: ldx = K + 8, out a column slice [16, 16 + N) of a (M, N + 32) buffer, h with sentinels.
    M = 394: device count 2 x 150 = 300 rows (tiles past it exit, the tile holding row 300 is partial).  Returns the whole
    output buffer, h, and the live row count."""
    x, gamma, beta, w, bias = _data(M, N, K, seed)
    flags = FLAG_SETS[kind](yv)
    f32 = bool(flags & yv.EPI_OUT_F32)
    xbuf = torch.full((M, K + 8), -9.0, device=DEV)
    xbuf[:, :K] = x.to(DEV)
    xd = xbuf[:, :K]
    h = torch.full((M, K), FILL, dtype=torch.bfloat16, device=DEV)
    obuf = torch.full((M, N + 32), FILL, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
    out = obuf[:, 16:16 + N]
    m_dev, mul, rows = (torch.tensor([2], dtype=torch.int32, device=DEV), 150, 300) if M == 394 else (None, 1, M)
    b = bias.to(DEV) if flags & yv.EPI_BIAS else None
    gd, bd, wd = gamma.to(DEV), beta.to(DEV), w.to(DEV)
    if fused:
        r = yv.linear_ln_route(M, N, K, flags)
        assert r.fused == 1 and (r.tiles_m, r.tiles_n, r.workgroups) == (-(-M // 64), N // 64, -(-M // 64) * (N // 64))
        yv.linear_ln(xd, gd, bd, h, wd, b, out, flags=flags & ~yv.EPI_BIAS, m_dev=m_dev, m_mul=mul)
    else:
        # yv_linear sends N <= 64 to its register-staged kernel whatever "linear_mid" says.  The mid route's 64 x 64 tile of
        # columns 0 .. 63 does not depend on the tiles beside it, so the pair runs on two column tiles - the same 64 weight rows
        # and 64 more - and its first tile is the reference.
        Np = 128 if N == 64 else N
        if Np != N:
            wd, obuf = torch.cat([wd, wd.flip(0)]), torch.cat([obuf, obuf[:, :Np - N]], 1)
            b = None if b is None else torch.cat([b, b])
        out = obuf[:, 16:16 + Np]
        r = yv.linear_route(M, Np, K, flags, lda=K, ldo=Np + 32, m_dev=m_dev is not None)
        assert (r.kernel, r.tile_rows, r.tile_cols) == (yv.LIN_MID, 64, 64)
        yv.layernorm(xd, gd, bd, h, M, K, K + 8, K, count_dev=m_dev, rows_per_count=mul)
        yv.linear(h, wd, b, out, flags=flags & ~yv.EPI_BIAS, m_dev=m_dev, m_mul=mul)
    torch.cuda.synchronize()
    return obuf.cpu(), h.cpu(), rows, (x, gamma, beta, w, bias)


@pytest.mark.parametrize("kind", list(FLAG_SETS))
@pytest.mark.parametrize("M,N,K", CASES)
def test_linear_ln_has_the_bits_of_the_pair(yv, M, N, K, kind):
    seed = M + N + K
    with every_shape(yv):
        got, h_fused, rows, ops = _run(yv, M, N, K, kind, True, seed)
        ref, h_pair, rows_ref, _ = _run(yv, M, N, K, kind, False, seed)
    assert rows == rows_ref
    assert torch.equal(got[:rows, 16:16 + N], ref[:rows, 16:16 + N])
    # not vacuous: the result is the product.  Against fp64 the bf16 rounding of the normalised operand and of the result (each
    # at most 2^-9 relative, 1.1e-3 rms) predict a rel-L2 of about 1.6e-3; the gate is four times that.
    x, gamma, beta, w, bias = ops
    xn = torch.nn.functional.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-6)
    lin = xn @ w.double().t()
    if kind != "plain":
        lin = lin + bias.double()
    if kind == "gelu":
        lin = torch.nn.functional.gelu(lin)
    err = rel_l2(got[:rows, 16:16 + N], lin[:rows])
    print(f"{M}x{N}x{K} {kind}: rel-L2 against fp64 {err:.3e}")
    assert err < 6.4e-3
    # nothing written outside the result: h, the rows at and past the device count, the columns beside the slice
    assert torch.equal(h_fused, torch.full_like(h_fused, FILL))
    assert not torch.equal(h_pair[:rows], torch.full_like(h_pair[:rows], FILL))
    assert torch.equal(got[rows:], torch.full_like(got[rows:], FILL))
    assert torch.equal(got[:, :16], torch.full_like(got[:, :16], FILL))
    assert torch.equal(got[:, 16 + N:], torch.full_like(got[:, 16 + N:], FILL))


def test_linear_ln_falls_back_to_the_pair(yv):
    """linear_ln_mid = 0 (the default): the same call is layernorm into h followed by linear."""
    M, N, K = 320, 192, 768
    assert yv.get_option("linear_ln_mid") == 0
    with options(yv, linear_mid=ROWS, linear_mid_fill=1 << 20):
        assert yv.linear_ln_route(M, N, K, yv.EPI_BIAS | yv.EPI_GELU).fused == 0
        x, gamma, beta, w, bias = (t.to(DEV) for t in _data(M, N, K, 11))
        h1 = torch.full((M, K), FILL, dtype=torch.bfloat16, device=DEV)
        h2 = h1.clone()
        o1 = torch.full((M, N), FILL, dtype=torch.bfloat16, device=DEV)
        o2 = o1.clone()
        yv.linear_ln(x, gamma, beta, h1, w, bias, o1, flags=yv.EPI_GELU)
        yv.layernorm(x, gamma, beta, h2, M, K, K, K)
        yv.linear(h2, w, bias, o2, flags=yv.EPI_GELU)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(h1, h2)
        assert not torch.equal(h1, torch.full_like(h1, FILL))
        with options(yv, linear_ln_mid=ROWS, linear_ln_fill=1 << 20):          # and the fused launch agrees with it
            assert yv.linear_ln_route(M, N, K, yv.EPI_BIAS | yv.EPI_GELU).fused == 1
            o3 = torch.full((M, N), FILL, dtype=torch.bfloat16, device=DEV)
            yv.linear_ln(x, gamma, beta, h2, w, bias, o3, flags=yv.EPI_GELU)
            torch.cuda.synchronize()
            assert torch.equal(o3, o1)


# ------------------------------------------------------------------------------------------------ engine
def _engine_inputs(name, cap, seed):
    from yvhip import engines
    sd = engines.init_vit_wrapper_state(name, NC, seed=2)
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randn(cap, 3, 224, 224, generator=g)
    P = engines.vit_cfg(name)[0]
    patches = torch.cat([torch.from_numpy(ob.patchify(imgs[r].numpy(), P)) for r in range(cap)])
    return sd, imgs, patches.to(torch.bfloat16).to(DEV)


def _logits(eng, patches, cap):
    logits = torch.zeros(cap, NC, device=DEV)
    labels = torch.zeros(cap, dtype=torch.int32, device=DEV)
    with eng.guard(0):
        feats = eng.backbone(patches, cap, None, 0)
        eng.head(feats, cap, logits, labels)
    torch.cuda.synchronize()
    return logits.cpu(), labels.cpu()


@pytest.mark.parametrize("name,cap,kw", [("vit_tiny_test", 2, dict(cls_tail=True)), ("vit_tiny_test", 2, dict(cls_tail=False)),
                                         ("vit_tiny_test", 4, dict(cls_tail=True)), ("vit_tiny_test", 4, dict(cls_tail=False)),
                                         ("vit_tiny8_test", 1, dict(long_attn=True))])
def test_engine_ln_gemm(yv, name, cap, kw):
    """With both fill rules raised, mid_gemm + ln_gemm logits have the bits of mid_gemm's (qkv and fc1 on 64 x 64 tiles in both);
    under the shipped options they are within rel-L2 2e-2 of oracle/vit.py in fp32 (the bound of tests/test_gpu_models.py) and
    the labels are their argmax.  The options are back at their values after every pass."""
    from yvhip import engines
    sd, imgs, patches = _engine_inputs(name, cap, 5)
    mid = engines.VitEngine(sd, name, NC, device=DEV, mid_gemm=True, ln_gemm=False, **kw)
    both = engines.VitEngine(sd, name, NC, device=DEV, mid_gemm=True, ln_gemm=True, **kw)
    M, D = cap * both.N, both.D
    assert 256 < M <= ROWS
    with options(yv, linear_mid_fill=1 << 20, linear_ln_fill=1 << 20):
        with options(yv, linear_mid=ROWS, linear_ln_mid=ROWS):                  # what the passes set
            for n, f in ((3 * D, 0), (4 * D, yv.EPI_GELU)):
                assert yv.linear_route(M, n, D, f | yv.EPI_BIAS, m_dev=False).kernel == yv.LIN_MID
                assert yv.linear_ln_route(M, n, D, f | yv.EPI_BIAS).fused == 1
        l_mid, _ = _logits(mid, patches, cap)
        l_both, _ = _logits(both, patches, cap)
        assert torch.equal(l_mid, l_both)
    assert yv.get_option("linear_ln_mid") == 0 and yv.get_option("linear_mid") == 0
    ref = ov.wrapper_forward(sd, imgs, name)
    for label, eng in (("ln_gemm", engines.VitEngine(sd, name, NC, device=DEV, ln_gemm=True, **kw)), ("mid_gemm + ln_gemm", both)):
        lg, lb = _logits(eng, patches, cap)
        err = rel_l2(lg, ref)
        print(f"{name} x {cap} {kw} {label}: rel-L2 against the fp32 oracle {err:.3e}")
        assert err < 2e-2
        assert lb.tolist() == lg.argmax(1).tolist()
    assert yv.get_option("linear_ln_mid") == 0


def test_engine_ln_gemm_refuses_fused_ln_and_mxfp8(yv):
    from yvhip import engines
    sd = engines.init_vit_wrapper_state("vit_tiny_test", NC, seed=2)
    with pytest.raises(yv.YvError, match="ln_gemm"):
        engines.VitEngine(sd, "vit_tiny_test", NC, device=DEV, fused_ln=True, ln_gemm=True)
    with pytest.raises(yv.YvError, match="ln_gemm"):
        engines.VitEngine(sd, "vit_tiny_test", NC, device=DEV, dtype="mxfp8", ln_gemm=True)


# ------------------------------------------------------------------------------------------------ pipeline
S, B, NAME = 128, 2, "vit_tiny_test"
FULL_KEYS = ("num_dets", "bboxes", "scores", "labels", "det_count", "crop_total")
LIVE_KEYS = ("det_box", "det_score", "det_label", "crop_rect", "crop_ok")


@pytest.fixture(scope="module")
def parts(yv):
    """The inputs of tests/test_gpu_fit_crops.py: engines, images, a conf threshold that leaves 3 .. 16 crops, the unflagged
    fit_crops result and the fp32 oracle logits of its crops."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    ysd = engines.init_yolo_state("n", NC, seed=1, head_gain=4.0)
    vsd = engines.init_vit_wrapper_state(NAME, NC, seed=2)
    yolo = engines.YoloEngine(ysd, "n", NC, S, DEV)
    vit = engines.VitEngine(vsd, NAME, NC, device=DEV, mid_gemm=False, ln_gemm=False)
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    imgd = img.to(DEV)
    probe = DetectClassifyPipeline(yolo, [vit], conf=0.0).detect_stage(imgd)
    scores = sorted((float(probe["det_score"][b, k]) for b in range(B) for k in range(int(probe["det_count"][b]))), reverse=True)
    conf, base = None, None
    for keep in (8, 6, 12, 4, 16, 3):
        if len(scores) <= keep or scores[keep - 1] == scores[keep]:
            continue
        c = 0.5 * (scores[keep - 1] + scores[keep])
        out = DetectClassifyPipeline(yolo, [vit], conf=c, fit_crops=True)(imgd)
        if 2 < int(out["crop_total"][0]) <= 16:
            conf, base = c, out
            break
    assert conf is not None, scores
    torch.cuda.synchronize()
    base = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in base.items()}
    total = int(base["crop_total"][0])
    ref = []
    for row in base["crop_list"][:total].tolist():
        x = torch.from_numpy(ob.crop_resize_normalize(img[row[0]].numpy(), row[1:5]))[None]
        ref.append(ov.wrapper_forward(vsd, x, NAME)[0])
    return dict(yolo=yolo, img=imgd, conf=conf, base=base, total=total, ref=torch.stack(ref), vsd=vsd)


@pytest.mark.parametrize("fill", [None, 1 << 20], ids=["shipped_fill", "every_shape_fused"])
@pytest.mark.parametrize("mid_gemm", [False, True])
def test_pipeline_with_ln_gemm_engines(yv, parts, mid_gemm, fill):
    """fill None: the shipped "linear_ln_fill" (no shape: linear_ln runs the pair); raised: the fused launches."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline, fit_capacity
    base, total = parts["base"], parts["total"]
    vit = engines.VitEngine(parts["vsd"], NAME, NC, device=DEV, mid_gemm=mid_gemm, ln_gemm=True)
    fill = yv.get_option("linear_ln_fill") if fill is None else fill
    with options(yv, linear_ln_fill=fill):
        with options(yv, linear_ln_mid=ROWS):
            M = fit_capacity(total, B * 100) * vit.N
            assert yv.linear_ln_route(M, 3 * vit.D, vit.D, yv.EPI_BIAS).fused == (fill > 0)
        out = DetectClassifyPipeline(parts["yolo"], [vit], conf=parts["conf"], fit_crops=True)(parts["img"])
        torch.cuda.synchronize()
    out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    for k in FULL_KEYS:
        assert torch.equal(out[k], base[k]), k
    for k in LIVE_KEYS:
        for b in range(B):
            n = int(base["det_count"][b])
            assert torch.equal(out[k][b, :n], base[k][b, :n]), (k, b)
    assert torch.equal(out["crop_list"][:total], base["crop_list"][:total])
    assert out["capacity"] == base["capacity"]
    assert yv.get_option("linear_ln_mid") == 0 and yv.get_option("linear_mid") == 0
    err = rel_l2(out["cls_logits"][:total], parts["ref"])
    print(f"ln_gemm, mid_gemm={mid_gemm}: rel-L2 of {total} crops' logits against the fp32 oracle {err:.3e}")
    assert err < 2e-2
    assert out["cls_label"][:total].tolist() == out["cls_logits"][:total].argmax(1).tolist()


def test_step_with_ln_gemm_is_graph_capturable(yv):
    """tests/test_gpu_models.py::test_step_is_graph_capturable with an ln_gemm classifier at request size (12 crop slots: 2,364
    rows; "linear_ln_fill" raised so that the fused launches run, carrying the device crop count): one capture on a single stream,
    replayed on new images, equals eager."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    fill = 1 << 20
    name, S, B = "vit_tiny_test", 128, 4
    vit = engines.VitEngine(engines.init_vit_wrapper_state(name, 5, 4), name, 5, device=DEV, mid_gemm=True, ln_gemm=True)
    pipe = DetectClassifyPipeline(engines.YoloEngine(engines.init_yolo_state("n", 5, 3, 4.0), "n", 5, S, DEV), [vit],
                                  max_crops_per_image=3)
    with options(yv, linear_ln_mid=ROWS, linear_ln_fill=fill):
        assert yv.linear_ln_route(B * 3 * vit.N, 3 * vit.D, vit.D, yv.EPI_BIAS).fused == 1
    g = torch.Generator().manual_seed(31)
    batches = [torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(3)]
    keys = ("det_count", "det_box", "crop_list", "crop_total", "cls_logits", "cls_label")
    ref = []
    with options(yv, linear_ln_fill=fill, linear_mid_fill=fill):   # (the route is decided on the host, at capture time)
        for im in batches:
            o = pipe(im)
            torch.cuda.synchronize()
            ref.append({k: o[k].clone() for k in keys})
        assert int(ref[0]["crop_total"][0]) > 0
        static = batches[0].clone()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                              # warm the capture stream's workspace registration
            pipe(static)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = pipe(static)
    for im, r in zip(batches, ref):
        static.copy_(im)
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(out[k], r[k]), k
    assert yv.get_option("linear_ln_mid") == 0
