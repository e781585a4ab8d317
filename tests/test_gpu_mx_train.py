"""MXFP8 fine-tune recipe on the device (VitTrainer(dtype="mxfp8")): the two-form quantiser byte for
byte, the MX training epilogues on both kernel instances against the fp64 product of the dequantised operands, the MX
weight gradient exactly, the trainer's gradients against an emulated-MX and an fp32 autograd, train / serve consistency
with VitEngine(dtype="mxfp8"), convergence on a learnable synthetic task, and the untouched bf16 default."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def r128(n):
    return (n + 127) // 128 * 128


# ------------------------------------------------------------------------------------------------ 1. quantiser
@pytest.mark.parametrize("T,C,ld", [(100, 128, 128), (197 * 3, 384, 512), (6304, 768, 768), (6304 * 2 + 37, 256, 384),
                                    (64, 3072, 3072)])
def test_quant_mxfp8_2d_is_byte_exact(yv, T, C, ld):
    g = torch.Generator().manual_seed(T + C)
    base = (torch.randn(T, ld, generator=g) * torch.exp(torch.randn(T, 1, generator=g) * 2)).to(torch.bfloat16)
    base[5] = 0                                                      # a row of zeros
    base[:, 32:64] = 0                                               # a column block of zeros
    xd = base.to(DEV)[:, ld - C:]                                    # strided view when ld > C
    q, s, qt, st = yv.quant_mxfp8_2d(xd)
    rq, rs = yv.quant_mxfp8(xd.contiguous())
    xt = torch.zeros(C, r128(T), dtype=torch.bfloat16, device=DEV)
    xt[:, :T] = xd.t()
    tq, ts = yv.quant_mxfp8(xt)
    torch.cuda.synchronize()
    assert torch.equal(q, rq) and torch.equal(s[:, :T], rs[:, :T])
    assert torch.equal(qt, tq) and torch.equal(st[:, :C], ts[:, :C])
    # one form only: the same bytes
    q1, s1, _, _ = yv.quant_mxfp8_2d(xd, col_form=False)
    _, _, qt1, st1 = yv.quant_mxfp8_2d(xd, row_form=False)
    torch.cuda.synchronize()
    assert torch.equal(q1, q) and torch.equal(s1, s) and torch.equal(qt1, qt) and torch.equal(st1, st)


# ------------------------------------------------------------------------------------------------ 2. epilogues
def _operands(yv, M, N, K, seed):
    from mx_reference import emulate_quant
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    ad = emulate_quant(a.float())[2].to(DEV)
    wd = emulate_quant(w.float())[2].to(DEV)
    ref = (ad @ wd.t()).cpu()                                         # fp64 product of the dequantised operands
    aq, asc = yv.quant_mxfp8(a.to(DEV))
    wq, wsc = yv.quant_mxfp8(w.to(DEV))
    return g, aq, asc, wq, wsc, bias, ref


_FLAGS = lambda yv: {"save_pre": yv.EPI_GELU | yv.EPI_SAVE_PRE, "res_src": yv.EPI_RES_F32, "gelu_bwd": yv.EPI_GELU_BWD}


def _epilogue_case(yv, kind, M, N, K, seed):
    """Runs one MX training epilogue, checks it against the fp64 product of the dequantised operands (the tolerances of
    test_gpu_fp8.py::test_linear_mxfp8_matches_dequantised_product) and returns its outputs (CPU)."""
    flags = _FLAGS(yv)[kind]
    bias_on = kind != "gelu_bwd"
    g, aq, asc, wq, wsc, bias, ref = _operands(yv, M, N, K, seed)
    lin = ref + (bias.double() if bias_on else 0.0)
    if kind == "save_pre":
        out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        pre = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        yv.linear_mxfp8_ex(aq, asc, wq, wsc, bias.to(DEV), out, flags=flags, aux=pre)
        torch.cuda.synchronize()
        e1, e2 = rel_l2(pre.cpu().float(), lin), rel_l2(out.cpu().float(), F.gelu(lin.float()))
        assert e1 < 4e-3 and e2 < 4e-3, (e1, e2)                     # bf16 output rounding
        return out.cpu(), pre.cpu()
    if kind == "res_src":
        x = torch.randn(M, N, generator=g)
        src = x.to(DEV)
        out = torch.full((M, N), 3.0, device=DEV)
        yv.linear_mxfp8_ex(aq, asc, wq, wsc, bias.to(DEV), out, flags=flags, res_f32=src)
        torch.cuda.synchronize()
        exp = x.double() + lin
        assert torch.allclose(out.cpu().double(), exp, rtol=2e-5, atol=2e-5 * float(exp.abs().max()))
        assert torch.equal(src.cpu(), x)                                # the source is read only
        return (out.cpu(),)
    u = (torch.randn(M, N, generator=g) * 2).to(torch.bfloat16)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    yv.linear_mxfp8_ex(aq, asc, wq, wsc, None, out, flags=flags, aux=u.to(DEV))
    torch.cuda.synchronize()
    ut = u.double().clone().requires_grad_(True)
    F.gelu(ut).backward(lin)                                            # lin * gelu'(u)
    err = rel_l2(out.cpu().float(), ut.grad)
    assert err < 4e-3, err
    return (out.cpu(),)


@pytest.mark.parametrize("kind,M,N,K,inst", [
    ("save_pre", 6304, 3072, 768, 1), ("save_pre", 6304, 768, 768, 0),            # fc1 forward forms (ViT-B/16, 32 crops)
    ("res_src", 12608, 768, 768, 1), ("res_src", 6304, 768, 768, 0),              # proj / fc2 forward (R = 64 / R = 32)
    ("gelu_bwd", 6304, 3072, 768, 1), ("gelu_bwd", 1000, 3072, 768, 0),           # fc2 data gradient
    ("save_pre", 6304, 4096, 1024, 1), ("gelu_bwd", 6304, 4096, 1024, 1),         # ViT-L/16 at 32 crops: 224-row tiles
    ("save_pre", 6304, 3072, 640, 1), ("gelu_bwd", 6304, 3072, 640, 1)])          # odd K / 128: 224-row tiles
def test_mx_linear_ex_epilogues(yv, kind, M, N, K, inst):
    bias_on = kind != "gelu_bwd"
    flags = _FLAGS(yv)[kind] | (yv.EPI_BIAS if bias_on else 0)
    assert yv.linear_mxfp8_instance(M, N, K, flags) == inst
    # the persistent kernel's tile height: 160 rows by the ViT-B/16 shapes, 224 by the ViT-L/16 shapes and by an odd K / 128
    r = yv.linear_route(M, N, K, flags, mx=True, res_f32=kind == "res_src", ldaux=0 if kind == "res_src" else N)
    rows = {(6304, 3072, 768): 160, (12608, 768, 768): 160, (6304, 4096, 1024): 224, (6304, 3072, 640): 224}
    if inst:
        assert (r.kernel, r.tile_rows, r.mx, r.ext, r.f32out) == (yv.LIN_P9, rows[M, N, K], 1, ["res_src", "save_pre", "gelu_bwd"].index(kind),
                                                                  int(kind == "res_src")), r
    else:
        assert (r.kernel, r.tile_rows, r.tile_cols, r.splitk) == (yv.LIN_MX, 128, 128, 1), r
    _epilogue_case(yv, kind, M, N, K, M + N + K + inst)


@pytest.mark.parametrize("kind", ["save_pre", "gelu_bwd"])
def test_mx_linear_ex_persistent_tile_heights(yv, kind):
    """Every tile height of the persistent kernel's trainer-epilogue instances (160 / 192 / 224 rows, forced through the
    "linear_p8_rows" option): correct, and the same bits as the height the launcher picks (one MFMA per K tile in K order
    whatever the height)."""
    M, N, K = 6304, 3072, 768
    prev = yv.get_option("linear_p8_rows")
    try:
        outs = {}
        for rows in (0, 160, 192, 224):
            yv.set_option("linear_p8_rows", rows)
            r = yv.linear_route(M, N, K, _FLAGS(yv)[kind] | (yv.EPI_BIAS if kind == "save_pre" else 0), mx=True, ldaux=N)
            assert (r.kernel, r.tile_rows, r.ext) == (yv.LIN_P9, rows if rows else 160, 1 if kind == "save_pre" else 2), r
            outs[rows] = _epilogue_case(yv, kind, M, N, K, 77)
    finally:
        yv.set_option("linear_p8_rows", prev)
    for rows in (160, 192, 224):
        assert all(torch.equal(a, b) for a, b in zip(outs[rows], outs[0])), rows


# ------------------------------------------------------------------------------------------------ 3. weight gradient
@pytest.mark.parametrize("T,N,K", [(6336, 2304, 768), (6400, 768, 3072), (1000, 256, 384)])
def test_wgrad_mxfp8_exact(yv, T, N, K):
    """Small-integer operands: every e4m3 value and every f32 sum is exact, so the result must EQUAL dY^T . X - a lane,
    swizzle, scale-row or token-order error cannot hide behind a tolerance."""
    g = torch.Generator().manual_seed(T + N + K)
    live = T - 37
    dy = torch.zeros(T, N); dy[:live] = torch.randint(-3, 4, (live, N), generator=g).float()
    x = torch.zeros(T, K); x[:live] = torch.randint(-2, 3, (live, K), generator=g).float()
    dy[:, :32] *= 8                                                     # blocks with different scales along N ...
    # ... and along the tokens: 32-token block b scaled by 2^(b % 3) (X) and 2^(b % 2) (dY), so neighbouring token blocks of a
    # row of X^T / dY^T carry different E8M0 exponents (values stay exact: at most two significant bits times a power of two)
    blk = torch.arange(T) // 32
    x *= (2.0 ** (blk % 3)).float()[:, None]
    dy *= (2.0 ** (blk % 2)).float()[:, None]
    ref = dy.t() @ x
    _, _, dyt, sdy = yv.quant_mxfp8_2d(dy.to(torch.bfloat16).to(DEV), row_form=False)
    _, _, xt, sx = yv.quant_mxfp8_2d(x.to(torch.bfloat16).to(DEV), row_form=False)
    outs = []
    prev = yv.get_option("wgrad_mx_split")
    try:
        for split in (0, 1, 3):                                         # auto, off, forced
            yv.set_option("wgrad_mx_split", split)
            dw = torch.full((N, K), 7.0, device=DEV)
            yv.wgrad_mxfp8(dyt, sdy, xt, sx, dw)
            outs.append(dw.cpu())
    finally:
        yv.set_option("wgrad_mx_split", prev)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], ref)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    # into a row-strided gradient buffer
    big = torch.full((N, K + 64), 5.0, device=DEV)
    yv.wgrad_mxfp8(dyt, sdy, xt, sx, big[:, :K])
    torch.cuda.synchronize()
    assert torch.equal(big[:, :K].cpu(), ref) and float(big[:, K:].sub(5.0).abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4. trainer gradients
def _patches(x, P):
    from oracle import boxes as ob
    return torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), P)) for r in range(x.shape[0])]).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("name,R", [("vit_tiny_test", 3), ("vit_tiny_test", 33), ("vit_tiny8_test", 2)])
def test_mx_trainer_gradients(yv, name, R):
    from oracle import vit as ov
    from yvhip.training import VitTrainer
    from test_gpu_configs import _relu_free_head
    from mx_train_emulation import grads
    sd = _relu_free_head(ov.init_wrapper_state(name, seed=21))
    g = torch.Generator().manual_seed(R)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32)
    _, _, emu = grads(sd, x, labels, name, mx=True)
    ref_loss, _, ref = grads(sd, x, labels, name, mx=False)
    tr = VitTrainer(sd, name, 5, dtype="mxfp8")
    pm = _patches(x, tr.P_)
    tr.forward(pm, R)
    loss = tr.backward(pm, labels.to(DEV), R)
    torch.cuda.synchronize()
    got = tr.grad_dict()
    e_emu = {k: rel_l2(got[k].cpu(), v) for k, v in emu.items()}
    e_ref = {k: rel_l2(got[k].cpu(), v) for k, v in ref.items()}
    c_ref = {k: cosine(got[k].cpu(), v) for k, v in ref.items()}
    worst = lambda d, sign=-1: sorted(d.items(), key=lambda kv: sign * kv[1])[:3]
    print(f"\n{name} R={R}: vs emulated MX worst rel-L2 {worst(e_emu)}; vs fp32 worst rel-L2 {worst(e_ref)}, "
          f"worst cosine {worst(c_ref, 1)}; loss {float(loss[0]):.5f} vs fp32 {float(ref_loss):.5f}")
    assert abs(float(loss[0]) - float(ref_loss)) < 3e-2 * abs(float(ref_loss))
    # measured worst cases over the three shapes: 0.062 against the emulation, 0.085 / cosine 0.9964
    # against fp32, all at the patch-embed weight (the end of the data-gradient chain); gates with ~30 % headroom
    assert max(e_emu.values()) <= 0.08, worst(e_emu)
    assert max(e_ref.values()) <= 0.12, worst(e_ref)
    assert min(c_ref.values()) >= 0.99, worst(c_ref, 1)


def test_mx_trainer_vit_b16_bench_shape(yv):
    """ViT-B/16 at R = 32 (M = 6,304: qkv / fc1 forward and the fc2 data gradient on the persistent instances): every block
    linear's weight gradient against the bf16 trainer's."""
    from yvhip import engines
    from yvhip.training import VitTrainer
    name, R = "vit_base_patch16_224", 32
    M = R * 197
    assert yv.linear_mxfp8_instance(M, 2304, 768, yv.EPI_BIAS) == 1
    assert yv.linear_mxfp8_instance(M, 3072, 768, yv.EPI_BIAS | yv.EPI_GELU | yv.EPI_SAVE_PRE) == 1
    assert yv.linear_mxfp8_instance(M, 3072, 768, yv.EPI_GELU_BWD) == 1
    sd = engines.init_vit_wrapper_state(name, 5, seed=4)
    g = torch.Generator().manual_seed(6)
    pm = (torch.rand(R * 196, 768, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(DEV)
    res = {}
    for dtype in ("bf16", "mxfp8"):
        tr = VitTrainer(sd, name, 5, dtype=dtype)
        tr.forward(pm, R)
        tr.backward(pm, labels, R)
        torch.cuda.synchronize()
        res[dtype] = {k: v for k, v in tr.grad_dict().items() if ".blocks." in k and k.endswith("weight") and ("attn" in k or "mlp" in k)}
        del tr
    cos = {k: cosine(res["mxfp8"][k], res["bf16"][k]) for k in res["bf16"]}
    ranked = sorted(cos.items(), key=lambda kv: kv[1])
    print("\nViT-B/16 R=32 MX vs bf16 weight gradients, worst cosine: " + ", ".join(f"{k} {c:.4f}" for k, c in ranked[:4]))
    assert ranked[0][1] >= 0.96, ranked[:4]                      # measured worst 0.975 (block 0 qkv)


# ------------------------------------------------------------------------------------------------ 5. train / serve
@pytest.mark.parametrize("name,R", [("vit_tiny_test", 33), ("vit_base_patch16_224", 32)])
def test_mx_trainer_forward_matches_mx_engine(yv, name, R):
    from yvhip import engines
    from yvhip.training import VitTrainer
    sd = engines.init_vit_wrapper_state(name, 5, seed=8)
    g = torch.Generator().manual_seed(R)
    P = engines.vit_cfg(name)[0]
    pm = (torch.rand(R * (224 // P) ** 2, 3 * P * P, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    tr = VitTrainer(sd, name, 5, dtype="mxfp8")
    got = tr.forward(pm, R).clone()
    eng = engines.VitEngine(sd, name, 5, device=DEV, dtype="mxfp8")
    feats = eng.backbone(pm, R)
    logits = torch.zeros(R, 5, device=DEV)
    lab = torch.zeros(R, dtype=torch.int32, device=DEV)
    eng.head(feats, R, logits, lab)
    torch.cuda.synchronize()
    err = rel_l2(got.cpu(), logits.cpu())
    print(f"\n{name} R={R}: MX trainer vs MX engine logits rel-L2 {err:.2e}, bit-equal {torch.equal(got, logits)}")
    # same kernel instances on both sides (the instance rule depends on the shape only), and the engine's fused producers
    # (LayerNorm / attention / fc1 writing the MX operand) equal producer + yv_quant_mxfp8 (test_gpu_fp8.py): bit for bit
    assert torch.equal(got, logits), err


# ------------------------------------------------------------------------------------------------ 6. convergence
def test_mx_trainer_converges_like_bf16(yv):
    import mx_train_emulation as m
    from yvhip.training import VitTrainer
    x, labels = m.synthetic_task()
    sd = m.task_init()
    labels_d = labels.to(DEV)
    out = {}
    for dtype in ("bf16", "mxfp8"):
        tr = VitTrainer(sd, m.TASK_NAME, 5, dtype=dtype)
        pm = _patches(x, tr.P_)
        losses = []
        for _ in range(m.TASK_STEPS):
            loss, _ = tr.step(pm, labels_d, m.TASK_LR)
            losses.append(loss)
        logits = tr.forward(pm, m.TASK_R)
        torch.cuda.synchronize()
        losses = [float(v[0]) for v in losses]
        acc = float((logits.argmax(1).cpu() == labels.long()).float().mean())
        out[dtype] = (losses, acc)
        print(f"\n{dtype}: loss {losses[0]:.4f} -> {losses[-1]:.4f}, accuracy {acc:.2f}")
    for dtype, (losses, acc) in out.items():
        assert acc >= m.TASK_ACC, (dtype, acc)
        assert losses[-1] <= m.TASK_LOSS_FRAC * losses[0], (dtype, losses[0], losses[-1])
    assert out["mxfp8"][0][-1] <= 1.5 * out["bf16"][0][-1]


# ------------------------------------------------------------------------------------------------ 7. default untouched
def test_bf16_dtype_is_the_default(yv):
    from oracle import vit as ov
    from yvhip.training import VitTrainer
    name, R = "vit_tiny_test", 3
    sd = ov.init_wrapper_state(name, seed=3)
    g = torch.Generator().manual_seed(1)
    pm = (torch.rand(R * 196, 768, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(DEV)
    gr = []
    for kw in ({}, {"dtype": "bf16"}):
        tr = VitTrainer(sd, name, 5, **kw)
        tr.forward(pm, R)
        tr.backward(pm, labels, R)
        torch.cuda.synchronize()
        gr.append(tr.grad_dict())
    assert all(torch.equal(gr[0][k], gr[1][k]) for k in gr[0])
