"""GPU checks of the long-sequence attention forward (yv_attention_long): the product against fp32 torch over every blocking edge
(key group, query block, tile seam, the straddling group), the online-softmax branches, isolation of crops and of rows past N,
the device-side crop count, independence of a crop's bits from the launch, the log2-sum-exp and the backward that consumes it,
the MXFP8 image, and VitEngine / PipelinedRunner / VitTrainer with long_attn=True.  Inputs are bf16-representable; the gates are
those of the tests of yv_attention (tests/test_gpu_dense.py) and of the engines they mirror."""
import functools

import pytest
import torch

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


def ref_attention(qkv, R, N, H, dtype=torch.float32):
    """softmax(Q K^T / 8) V in `dtype` on the CPU -> (out (R*N, H*64), log2-sum-exp (R, H, N))."""
    t = qkv.to(dtype).view(R, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] * 0.125) @ t[1].transpose(-2, -1)
    out = (s.softmax(-1) @ t[2]).transpose(1, 2).reshape(R * N, H * 64)
    return out, torch.logsumexp(s, -1) * 1.4426950408889634


def run_long(yv, qkv, R, N, H, **kw):
    out = torch.zeros(R * N, H * 64, dtype=torch.bfloat16, device=DEV)
    yv.attention_long(qkv.to(DEV), R, N, H, out, **kw)
    torch.cuda.synchronize()
    return out.cpu().float()


def gates(got, ref):
    """Both gates of test_gpu_dense.py::test_attention (P is rounded to bf16 before P.V and the output to bf16: 2^-8 each)."""
    assert bool(torch.isfinite(got).all())
    err = rel_l2(got, ref)
    assert err < 8e-3, err
    assert torch.allclose(got, ref, atol=3e-2, rtol=2e-2)


# ------------------------------------------------------------------------------------------------ 1. against fp32 torch
SHAPES = [(1, 1, 1), (2, 5, 2), (2, 33, 1), (1, 128, 2), (2, 129, 1), (1, 225, 1), (1, 256, 3), (1, 257, 2), (1, 512, 1),
          (2, 577, 2), (2, 785, 3), (1, 897, 1), (1, 1000, 2), (3, 785, 12)]


@pytest.mark.parametrize("R,N,H", SHAPES)
def test_attention_long(yv, R, N, H):
    g = torch.Generator().manual_seed(R * 7 + N)
    qkv = bf(torch.randn(R * N, 3 * H * 64, generator=g) * 1.5)
    gates(run_long(yv, qkv, R, N, H), ref_attention(qkv, R, N, H)[0])


# ------------------------------------------------------------------------------------------------ 2. online-softmax branches
def _monotone_qkv(sign):
    """N = 785, H = 1: the scaled score of (query i, key j) is sign * c_i * j / 256 with c_i in {1, 1.5, 2, 2.5}, exactly (every
    product and sum is exact in f32): strictly monotone in the key index, a range of 3 .. 7.7 in the exponent - a well conditioned
    softmax."""
    N = 785
    g = torch.Generator().manual_seed(17)
    qkv = torch.zeros(N, 192)
    j = torch.arange(N)
    qkv[:, 0] = qkv[:, 1] = 1 + (j % 4) * 0.5                                  # q: two live columns
    qkv[:, 64] = sign * (j // 32).float()                                      # k: j / 32 split into two bf16-exact parts
    qkv[:, 65] = sign * (j % 32).float() / 32
    qkv[:, 128:] = torch.randn(N, 64, generator=g)
    qkv = bf(qkv)
    s = qkv[:, :64].float() @ qkv[:, 64:128].float().t()
    d = s[:, 1:] - s[:, :-1]
    assert bool((d * sign > 0).all())
    return qkv


def test_attention_long_ascending_scores(yv):
    """Every key group raises every query's maximum: O is rescaled in each of the 25 groups."""
    qkv = _monotone_qkv(1.0)
    gates(run_long(yv, qkv, 1, 785, 1), ref_attention(qkv, 1, 785, 1)[0])


def test_attention_long_descending_scores(yv):
    """The maximum is met in group 0: no rescale after it."""
    qkv = _monotone_qkv(-1.0)
    gates(run_long(yv, qkv, 1, 785, 1), ref_attention(qkv, 1, 785, 1)[0])


def test_attention_long_softmax_spike(yv):
    """One key dominates a query: key 0, key 784 (the last live key of the masked group) and keys 255 / 256 (a tile seam)."""
    R, N, H = 1, 785, 1
    g = torch.Generator().manual_seed(5)
    qkv = bf(torch.randn(N, 192, generator=g))
    pairs = ((7, 0), (100, 784), (300, 255), (500, 256))
    # |q| = |k| = 8 in every column; pair n flips the sign of its own 16 columns, so a spiked query scores 512 on its own key and
    # exactly 0 on the other pairs' keys
    for n, (qi, kj) in enumerate(pairs):
        sgn = torch.ones(64)
        sgn[16 * n:16 * n + 16] = -1.0
        qkv[qi, :64] = bf(8.0 * sgn)
        qkv[kj, 64:128] = bf(8.0 * sgn)
    ref = ref_attention(qkv, R, N, H)[0]
    got = run_long(yv, qkv, R, N, H)
    assert bool(torch.isfinite(got).all())
    assert torch.allclose(got, ref, atol=3e-2, rtol=2e-2)
    for qi, kj in pairs:
        assert torch.allclose(got[qi], qkv.float()[kj, 128:], atol=2e-2), (qi, kj)


# ------------------------------------------------------------------------------------------------ 3. no leak
@pytest.mark.parametrize("bad", [1, 0])
def test_attention_long_no_leak_across_crops(yv, bad):
    R, N, H = 2, 785, 2
    g = torch.Generator().manual_seed(31)
    qkv = bf(torch.randn(R * N, 3 * H * 64, generator=g) * 1.5)
    good = 1 - bad
    ref = ref_attention(qkv[good * N:(good + 1) * N], 1, N, H)[0]
    qkv[bad * N:(bad + 1) * N] = float("nan")
    got = run_long(yv, qkv, R, N, H)
    gates(got[good * N:(good + 1) * N], ref)


# ------------------------------------------------------------------------------------------------ 4. device-side count
@pytest.mark.parametrize("count", [2, 0, 5])
def test_attention_long_device_count(yv, count):
    R, N, H = 3, 257, 2
    D = H * 64
    g = torch.Generator().manual_seed(41)
    qkv = bf(torch.randn(R * N, 3 * D, generator=g)).to(DEV)
    rp = (R * N + 255) // 256 * 256

    def run(r_dev):
        out = torch.full((R * N, D), 1.5, dtype=torch.bfloat16, device=DEV)
        lse = torch.full((R * H * N,), 3.25, device=DEV)
        q = torch.full((R * N, D), 0xA5, dtype=torch.uint8, device=DEV)
        s = torch.full((D // 128, rp, 4), 0x5B, dtype=torch.uint8, device=DEV)
        yv.attention_long(qkv, R, N, H, out, r_dev=r_dev, lse=lse, out_q=q, out_scale=s)
        torch.cuda.synchronize()
        return out, lse, q, s

    full = run(None)
    got = run(torch.tensor([count], dtype=torch.int32, device=DEV))
    live = min(count, R)
    rows = live * N
    for a, b in zip(got[:3], full[:3]):                                        # out, lse ((r, h, n): crop-major), q
        n = rows if a.dim() == 2 else live * H * N
        assert torch.equal(a[:n], b[:n])
    assert torch.equal(got[3][:, :rows], full[3][:, :rows])
    assert bool((got[0][rows:] == 1.5).all()) and bool((got[1][live * H * N:] == 3.25).all())
    assert bool((got[2][rows:] == 0xA5).all()) and bool((got[3][:, rows:] == 0x5B).all())
    assert bool((full[3][:, R * N:] == 0x5B).all())                            # rows past R N belong to nobody
    if live:
        assert bool(torch.isfinite(got[0][:rows].float()).all())


# ------------------------------------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("N", [257, 785])
def test_attention_long_crop_bits_do_not_depend_on_the_launch(yv, N):
    R, H = 3, 2
    g = torch.Generator().manual_seed(N)
    qkv = bf(torch.randn(R * N, 3 * H * 64, generator=g) * 1.5)
    whole = run_long(yv, qkv, R, N, H)
    for r in range(R):
        alone = run_long(yv, qkv[r * N:(r + 1) * N].contiguous(), 1, N, H)
        assert torch.equal(whole[r * N:(r + 1) * N], alone), r


# ------------------------------------------------------------------------------------------------ 6. lse
@pytest.mark.parametrize("R,N,H", [(2, 785, 2), (1, 257, 1), (1, 600, 1)])
def test_attention_long_lse_and_backward(yv, R, N, H):
    """attention_bwd fed with attention_long's out and lse against fp32 autograd (the gate of test_gpu_train.py::
    test_attention_bwd), and the lse itself against the fp64 log2-sum-exp: both forwards make f32 sums of the same terms in
    another order, so attention_long may be 4 x as far off as attention_train plus 2^-20; a wrong running maximum or a missed
    rescale is an error of order 1.  Measured on an MI355X (max |lse - fp64|, attention_long / attention_train):
    (2, 785, 2) 1.74e-6 / 1.26e-6, (1, 257, 1) 1.28e-6 / 1.05e-6, (1, 600, 1) 1.32e-6 / 1.33e-6."""
    g = torch.Generator().manual_seed(R + N)
    D = H * 64
    qkv = bf(torch.randn(R * N, 3 * D, generator=g))
    do = bf(torch.randn(R * N, D, generator=g))
    t = qkv.float().clone().requires_grad_(True)
    tt = t.view(R, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref_o = (((tt[0] * 0.125) @ tt[1].transpose(-2, -1)).softmax(-1) @ tt[2]).transpose(1, 2).reshape(R * N, D)
    ref_o.backward(do.float())
    qd = qkv.to(DEV)
    out = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV); lse = torch.zeros(R * H * N, device=DEV)
    yv.attention_long(qd, R, N, H, out, lse=lse)
    assert rel_l2(out.cpu().float(), ref_o.detach()) < 8e-3
    dqkv = torch.zeros(R * N, 3 * D, dtype=torch.bfloat16, device=DEV); dws = torch.zeros(R * H * N, device=DEV)
    yv.attention_bwd(qd, out, do.to(DEV), lse, R, N, H, dqkv, dws)
    got = dqkv.cpu().float()
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert rel_l2(got[:, sl], t.grad[:, sl]) < 2e-2, name
    out_t = torch.zeros_like(out); lse_t = torch.zeros_like(lse)
    yv.attention_train(qd, R, N, H, out_t, lse_t)
    torch.cuda.synchronize()
    ref64 = ref_attention(qkv, R, N, H, torch.float64)[1].reshape(-1)
    e_long = float((lse.cpu().double() - ref64).abs().max())
    e_train = float((lse_t.cpu().double() - ref64).abs().max())
    print(f"\nlse R={R} N={N} H={H}: max |attention_long - fp64| {e_long:.3e}, max |attention_train - fp64| {e_train:.3e}")
    assert e_long <= 4 * e_train + 2.0 ** -20, (e_long, e_train)


# ------------------------------------------------------------------------------------------------ 7. MXFP8 image
@pytest.mark.parametrize("R,N,H", [(1, 785, 4), (2, 257, 2), (2, 50, 2)])
def test_attention_long_mxfp8_equals_out_then_quant(yv, R, N, H):
    """The contract of test_gpu_fp8.py::test_attention_mxfp8_equals_attention_then_quant: identical bytes and scales to the bf16
    output followed by yv_quant_mxfp8 on the live rows, rows past the device-side count untouched."""
    g = torch.Generator().manual_seed(R * 1000 + N + H)
    D = H * 64
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    cnt = torch.tensor([max(R - 1, 1)], dtype=torch.int32, device=DEV)
    live = int(cnt[0]) * N
    o = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    yv.attention_long(qkv, R, N, H, o, r_dev=cnt)
    q_ref, s_ref = yv.quant_mxfp8(o)
    q = torch.full((R * N, D), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full_like(s_ref, 0x5B)
    yv.attention_long(qkv, R, N, H, r_dev=cnt, out_q=q, out_scale=s)
    torch.cuda.synchronize()
    assert torch.equal(q[:live], q_ref[:live]) and torch.equal(s[:, :live], s_ref[:, :live])
    assert bool((q[live:] == 0xA5).all()) and bool((s[:, live:] == 0x5B).all())


def test_attention_long_mxfp8_zero_head(yv):
    """V of one head is zero: that head's two blocks of every row are all-zero blocks - scale byte 0, zero bytes (the -127 branch of
    the block exponent, csrc/mx_quant.h); the other heads equal the bf16 output followed by yv_quant_mxfp8."""
    R, N, H, zh = 1, 785, 4, 1
    D = H * 64
    g = torch.Generator().manual_seed(R * 1000 + N + H + 1)
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 0.7).to(torch.bfloat16)
    qkv[:, 2 * D + zh * 64:2 * D + (zh + 1) * 64] = 0
    qkv = qkv.to(DEV)
    o = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    yv.attention_long(qkv, R, N, H, o)
    q_ref, s_ref = yv.quant_mxfp8(o)
    q = torch.full((R * N, D), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full_like(s_ref, 0x5B)
    yv.attention_long(qkv, R, N, H, out_q=q, out_scale=s)
    torch.cuda.synchronize()
    assert bool((q[:, zh * 64:(zh + 1) * 64] == 0).all())
    s_rows = s[:, :R * N].permute(1, 0, 2).reshape(R * N, D // 32)
    assert bool((s_rows[:, 2 * zh:2 * zh + 2] == 0).all())
    assert torch.equal(q, q_ref) and torch.equal(s[:, :R * N], s_ref[:, :R * N])


# ------------------------------------------------------------------------------------------------ 8. engine
@functools.lru_cache(maxsize=None)
def _engine_case(name, R):
    """Weights, crops, the fp32 oracle and the default bf16 engine's outputs of one (model, crop count): computed once."""
    from oracle import boxes as ob, vit as ov
    sd = ov.init_wrapper_state(name, seed=11)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    ref_feats = ov.vit_forward(sd, x, name)
    ref_logits = ov.wrapper_head(sd, ref_feats)
    P = {"vit_tiny8_test": 8, "vit_base_patch8_224": 8}[name]
    pm = torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), P)) for r in range(R)]).to(torch.bfloat16)
    base = _run_engine(sd, name, R, pm)
    return sd, pm, ref_feats, ref_logits, base


def _run_engine(sd, name, R, pm, **kw):
    from yvhip import engines
    eng = engines.VitEngine(sd, name, 5, **kw)
    cap = R + 1                                      # one spare slot: dynamic count leaves it untouched
    buf = eng.patch_buffer(cap)
    buf[:pm.shape[0]] = pm.to(DEV)
    cnt = torch.tensor([R], dtype=torch.int32, device=DEV)
    feats = eng.backbone(buf, cap, cnt)
    logits = torch.zeros(cap, 5, device=DEV); labels = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    eng.head(feats, cap, logits, labels, count=cnt)
    torch.cuda.synchronize()
    assert eng.long_attn is bool(kw.get("long_attn", False))
    return feats.cpu(), logits.cpu(), labels.cpu()


ENGINE_CASES = [("vit_tiny8_test", 2), ("vit_base_patch8_224", 1)]


@pytest.mark.parametrize("fused_ln", [False, True])
@pytest.mark.parametrize("name,R", ENGINE_CASES)
def test_vit_engine_long_attn_vs_oracle(name, R, fused_ln):
    """Body and gates of test_gpu_models.py::test_vit_engine_vs_oracle with long_attn=True (also together with fused_ln), and
    the labels of the default engine where the oracle's margin is sure."""
    sd, pm, ref_feats, ref_logits, base = _engine_case(name, R)
    feats, logits, labels = _run_engine(sd, name, R, pm, long_attn=True, fused_ln=fused_ln)
    assert rel_l2(feats[:R, :1000], ref_feats) < 2e-2
    assert rel_l2(logits[:R], ref_logits) < 2e-2
    assert float(feats[:R, 1000:].abs().sum()) == 0
    assert int(labels[R]) == -1 and float(logits[R].abs().sum()) == 0
    margin = ref_logits.topk(2, 1).values
    sure = (margin[:, 0] - margin[:, 1]) > 0.05 * ref_logits.abs().max()
    assert labels[:R][sure].tolist() == ref_logits.argmax(1)[sure].tolist()
    assert labels[:R][sure].tolist() == base[2][:R][sure].tolist()


@pytest.mark.parametrize("name,R", ENGINE_CASES)
def test_vit_engine_long_attn_mxfp8(name, R):
    """dtype="mxfp8" with long_attn=True under the gates of test_gpu_fp8.py::test_vit_engine_mxfp8_tracks_bf16 (against the bf16
    engine on the same weights and crops: backbone logits rel-L2 < 0.12, per-crop cosine > 0.99, arg-max agreement >= 0.5), the
    spare slot untouched."""
    sd, pm, _, _, base = _engine_case(name, R)
    feats, logits, labels = _run_engine(sd, name, R, pm, long_attn=True, dtype="mxfp8")
    a, b = feats[:R, :1000].double(), base[0][:R, :1000].double()
    err = float((a - b).norm() / b.norm())
    agree = float((a.argmax(1) == b.argmax(1)).float().mean())
    cos = torch.nn.functional.cosine_similarity(a, b, dim=1)
    print(f"\n{name} R={R} mxfp8 + long_attn vs bf16: rel-L2 {err:.4f}, min cosine {float(cos.min()):.4f}, arg-max agreement {agree:.2f}")
    assert bool(torch.isfinite(a).all())
    assert err < 0.12, err
    assert float(cos.min()) > 0.99, float(cos.min())
    assert agree >= 0.5, agree
    assert int(labels[R]) == -1 and float(logits[R].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ 9. pipeline
def test_pipelined_runner_long_attn_matches_single_stream():
    """A long_attn engine (785 tokens) through PipelinedRunner(split_classifier=True) equals the same engine single-stream bit for
    bit (the check of test_gpu_fused_ln.py for its engine)."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline, PipelinedRunner
    name, S, B = "vit_tiny8_test", 128, 4
    vit = engines.VitEngine(engines.init_vit_wrapper_state(name, 5, 4), name, 5, device=DEV, long_attn=True)
    assert vit.long_attn and vit.N == 785
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


# ------------------------------------------------------------------------------------------------ 10. trainer
def test_trainer_long_attn_gradients_vs_autograd(yv):
    """Body and 2e-2 gates of test_gpu_train.py::test_trainer_gradients_vs_autograd with VitTrainer(long_attn=True)."""
    import torch.nn.functional as F
    from oracle import boxes as ob, train as ot, vit as ov
    from yvhip.training import VitTrainer
    from test_gpu_configs import _relu_free_head      # ReLU coin flips of the wrapper head taken out (see its docstring)
    name, R = "vit_tiny8_test", 2
    sd = _relu_free_head(ov.init_wrapper_state(name, seed=21))
    g = torch.Generator().manual_seed(R)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_logits = ov.wrapper_forward(p, x, name)
    ref_loss = ot.build_loss(ref_logits, F.one_hot(labels.long(), 5).float())
    ref_loss.backward()
    ref_loss, ref_logits, ref = ref_loss.detach(), ref_logits.detach(), {k: v.grad for k, v in p.items()}
    tr = VitTrainer(sd, name, 5, long_attn=True)
    assert tr.long_attn and tr.N == 785
    pm = torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), tr.P_)) for r in range(R)]).to(torch.bfloat16).to(DEV)
    logits = tr.forward(pm, R)
    loss = tr.backward(pm, labels.to(DEV), R)
    torch.cuda.synchronize()
    assert rel_l2(logits.cpu(), ref_logits) < 2e-2
    assert abs(float(loss[0]) - float(ref_loss)) < 2e-2 * abs(float(ref_loss))
    got = tr.grad_dict()
    worst = {k: rel_l2(got[k].cpu(), v) for k, v in ref.items()}
    ranked = sorted(worst.items(), key=lambda kv: -kv[1])
    print(f"\n{name} R={R} long_attn: gradient rel-L2 vs fp32 autograd, worst: " + ", ".join(f"{k} {e:.3f}" for k, e in ranked[:4]))
    bad = {k: e for k, e in worst.items() if e > 2e-2}
    assert not bad, bad
