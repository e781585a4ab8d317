"""GPU checks of the trainer's cls-row tail: yv_attention_cls_train against yv_attention_cls (bits) and the
fp32 log-sum-exp, yv_attention_cls_bwd against fp32 autograd of the query-0 formula and against yv_attention_bwd fed the scattered
gradient, and VitTrainer(cls_tail=True) against fp32 autograd with the gates of the full trainer's tests, in both recipes, plus its
structure (which launchers run, determinism, a full step, the flag's semantics, the default left alone)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def bf(t):
    return t.to(torch.bfloat16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _r64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ 1. the two kernels
# N below one 32-row trip, on and just past a trip boundary, both model lengths
SHAPES = [(2, 197, 3), (2, 5, 2), (1, 33, 1), (1, 64, 2), (1, 256, 2), (1, 257, 1), (2, 785, 2), (1, 1000, 1)]
SENTINEL, TAIL_ROWS = 7.0, 3


@functools.lru_cache(maxsize=None)
def _inputs(R, N, H):
    g = torch.Generator().manual_seed(R * 7 + N)
    D = H * 64
    return bf(torch.randn(R * N, 3 * D, generator=g)), bf(torch.randn(R, D, generator=g))


def _compact(q):
    """q in a buffer of its own with row stride H*64 (.contiguous() hands a one-row view back as it is, stride and all)."""
    return torch.empty(q.shape, dtype=q.dtype, device=q.device).copy_(q)


def _autograd(qkv, dout, R, N, H):
    """fp32 autograd of the query-0 formula: (out (R, D), d qkv (R*N, 3D))."""
    from test_gpu_cls_tail import _att_ref
    t = qkv.float().clone().requires_grad_(True)
    out = _att_ref(t, R, N, H)
    out.backward(dout.float())
    return out.detach(), t.grad


def _run_fwd(yv, q, qd, R, N, H):
    D = H * 64
    out = torch.full((R, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((R * H,), SENTINEL, device=DEV)
    yv.attention_cls_train(q, qd, R, N, H, out, lse)
    return out, lse


def _run_bwd(yv, q, qd, dout, lse, R, N, H):
    """dqkv with TAIL_ROWS sentinel rows past R*N; everything is pre-filled, so an unwritten element shows."""
    dqkv = torch.full((R * N + TAIL_ROWS, 3 * H * 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
    yv.attention_cls_bwd(q, qd, dout, lse, R, N, H, dqkv)
    torch.cuda.synchronize()
    return dqkv


def _check_grads(got, ref, R, N, D, what):
    """got (R*N, 3D) f32 from the kernel, ref the reference gradient: dq (cls rows), dk, dv each within rel-L2 2e-2 (the gate of
    test_gpu_train.py::test_attention_bwd)."""
    errs = {"dq": rel_l2(got[::N, :D], ref[::N, :D]), "dk": rel_l2(got[:, D:2 * D], ref[:, D:2 * D]),
            "dv": rel_l2(got[:, 2 * D:], ref[:, 2 * D:])}
    print(f"attention_cls_bwd {what}: rel-L2 " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < 2e-2, (what, k, e)


@pytest.mark.parametrize("R,N,H", SHAPES)
def test_attention_cls_train_forward(yv, R, N, H):
    qkv, _ = _inputs(R, N, H)
    D = H * 64
    qd = qkv.to(DEV)
    q_view, q_compact = qd[::N, :D], _compact(qd[::N, :D])
    assert q_view.stride(0) == N * 3 * D and q_compact.stride(0) == D
    ref_out = torch.zeros(R, D, dtype=torch.bfloat16, device=DEV)
    yv.attention_cls(q_compact, qd, R, N, H, ref_out)
    t = qkv.float().view(R, N, 3, H, 64)
    s = torch.einsum("rhd,rnhd->rhn", t[:, 0, 0], t[:, :, 1]) * 0.125                     # natural-log domain scores of query 0
    lse_ref = (torch.logsumexp(s, -1) * LOG2E).reshape(R * H)
    full = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    lse_full = torch.zeros(R * H * N, device=DEV)
    yv.attention_train(qd, R, N, H, full, lse_full)
    for q in (q_view, q_compact):
        out, lse = _run_fwd(yv, q, qd, R, N, H)
        torch.cuda.synchronize()
        assert torch.equal(out, ref_out)                                                 # the bits of yv_attention_cls
        e_ref = float((lse.cpu() - lse_ref).abs().max())
        e_train = float((lse - lse_full.view(R * H, N)[:, 0]).abs().max())
        print(f"attention_cls_train R={R} N={N} H={H}: |lse - fp32| {e_ref:.2e}, |lse - attention_train| {e_train:.2e}")
        assert e_ref < 1e-3 and e_train < 1e-3


@pytest.mark.parametrize("R,N,H", SHAPES)
def test_attention_cls_bwd(yv, R, N, H):
    qkv, dout = _inputs(R, N, H)
    D, M = H * 64, R * N
    _, ref = _autograd(qkv, dout, R, N, H)
    qd, dod = qkv.to(DEV), dout.to(DEV)
    q = qd[::N, :D]
    _, lse = _run_fwd(yv, q, qd, R, N, H)
    dqkv = _run_bwd(yv, q, qd, dod, lse, R, N, H)
    got = dqkv.cpu().float()
    assert bool(torch.isfinite(got).all())
    _check_grads(got[:M], ref, R, N, D, f"R={R} N={N} H={H} vs fp32 autograd")
    other = torch.ones(M, dtype=torch.bool)
    other[::N] = False
    assert float(got[:M][other][:, :D].abs().max() if other.any() else 0.0) == 0.0        # the Q third of every non-cls row: exactly 0
    assert torch.equal(got[M:], torch.full((TAIL_ROWS, 3 * D), SENTINEL))                 # nothing past row R*N
    assert torch.equal(_run_bwd(yv, q, qd, dod, lse, R, N, H), dqkv)                     # two runs: the same bits
    assert torch.equal(_run_bwd(yv, _compact(q), qd, dod, lse, R, N, H), dqkv)         # compact q: the same bits
    # the full backward fed the scattered gradient (zeros outside the cls rows)
    out_f = torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    lse_f = torch.zeros(R * H * N, device=DEV)
    yv.attention_train(qd, R, N, H, out_f, lse_f)
    do_f = torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    do_f[::N] = dod
    dq_f = torch.zeros(M, 3 * D, dtype=torch.bfloat16, device=DEV)
    yv.attention_bwd(qd, out_f, do_f, lse_f, R, N, H, dq_f, torch.zeros(R * H * N, device=DEV))
    _check_grads(got[:M], dq_f.cpu().float(), R, N, D, f"R={R} N={N} H={H} vs attention_bwd")


@pytest.mark.parametrize("N", [5, 197, 257])
def test_attention_cls_bwd_crop_bits_do_not_depend_on_the_launch(yv, N):
    R, H = 2, 2
    qkv, dout = _inputs(R, N, H)
    D = H * 64
    qd, dod = qkv.to(DEV), dout.to(DEV)
    out, lse = _run_fwd(yv, qd[::N, :D], qd, R, N, H)
    both = _run_bwd(yv, qd[::N, :D], qd, dod, lse, R, N, H)
    q1 = qd[N:].contiguous()                                                              # crop 1 alone
    out1, lse1 = _run_fwd(yv, q1[::N, :D], q1, 1, N, H)
    alone = _run_bwd(yv, q1[::N, :D], q1, dod[1:].contiguous(), lse1, 1, N, H)
    assert torch.equal(out1, out[1:]) and torch.equal(lse1, lse[H:])
    assert torch.equal(alone[:N], both[N:2 * N])


def test_attention_cls_bwd_softmax_spike(yv):
    # the case of test_gpu_cls_tail.py::test_attention_cls_softmax_spike: one key dominates the cls query
    R, N, H = 1, 197, 1
    g = torch.Generator().manual_seed(5)
    qkv = bf(torch.randn(N, 192, generator=g))
    qkv[0, :64] = 8.0; qkv[100, 64:128] = 8.0
    dout = bf(torch.randn(1, 64, generator=g))
    _, ref = _autograd(qkv, dout, R, N, H)
    qd, dod = qkv.to(DEV), dout.to(DEV)
    _, lse = _run_fwd(yv, qd[:1, :64], qd, R, N, H)
    got = _run_bwd(yv, qd[:1, :64], qd, dod, lse, R, N, H).cpu().float()[:N]
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(lse).all())
    _check_grads(got, ref, R, N, 64, "spike vs fp32 autograd")


# ------------------------------------------------------------------------------------------------ 2. trainer against fp32 autograd
@functools.lru_cache(maxsize=None)
def _problem(name, R):
    """Weights, crops, labels and the fp32 autograd reference of one case: computed once, shared, never modified."""
    from oracle import boxes as ob, vit as ov
    from test_gpu_configs import _relu_free_head      # ReLU coin flips of the wrapper head taken out (see its docstring)
    from test_gpu_train import _oracle_grads
    from yvhip import engines
    sd = _relu_free_head(ov.init_wrapper_state(name, seed=21))
    g = torch.Generator().manual_seed(R)
    x = (torch.rand(R, 3, 224, 224, generator=g) * 2 - 1).to(torch.bfloat16).float()
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32)
    ref_loss, ref_logits, ref = _oracle_grads(sd, x, labels, name)
    P = engines.vit_cfg(name)[0]
    pm = torch.cat([torch.from_numpy(ob.patchify(x[r].numpy(), P)) for r in range(R)]).to(torch.bfloat16).to(DEV)
    return sd, pm, labels.to(DEV), ref_loss, ref_logits, ref


def _train(name, R, **kw):
    """One forward + backward of a fresh trainer -> (trainer, logits, loss, gradients)."""
    from yvhip.training import VitTrainer
    sd, pm, labels = _problem(name, R)[:3]
    tr = VitTrainer(sd, name, 5, **kw)
    logits = tr.forward(pm, R).clone()
    loss = tr.backward(pm, labels, R).clone()
    torch.cuda.synchronize()
    return tr, logits, loss, tr.grad_dict()


def _tail_errors(name, R, **kw):
    """(trainer, logits, loss, {tensor: rel-L2 vs fp32 autograd}) of the cls-tail trainer; prints rel-L2(tail, full) per tensor
    against the full trainer of the same flags (recorded in DESIGN.md section 17, not gated)."""
    ref = _problem(name, R)[5]
    tr, logits, loss, got = _train(name, R, cls_tail=True, **kw)
    assert tr.cls_tail is True
    full = _train(name, R, cls_tail=False, **kw)[3]
    err = {k: rel_l2(got[k].cpu(), v) for k, v in ref.items()}
    vs_full = sorted(((k, rel_l2(got[k], full[k])) for k in ref), key=lambda kv: -kv[1])
    vals = sorted(e for _, e in vs_full)
    print(f"\n{name} R={R} {kw}: rel-L2(tail, full) median {vals[len(vals) // 2]:.4f}, worst: "
          + ", ".join(f"{k} {e:.4f}" for k, e in vs_full[:4]))
    ranked = sorted(err.items(), key=lambda kv: -kv[1])
    print(f"{name} R={R} {kw}: gradient rel-L2 vs fp32 autograd, worst: " + ", ".join(f"{k} {e:.4f}" for k, e in ranked[:4]))
    return tr, logits, loss, err


@pytest.mark.parametrize("name,R,kw", [("vit_tiny_test", 3, {}), ("vit_tiny_test", 33, {}), ("vit_tiny8_test", 2, {}),
                                       ("vit_tiny8_test", 2, dict(long_attn=True, long_attn_bwd=True))])
def test_cls_tail_trainer_gradients_vs_autograd(yv, name, R, kw):
    """The body and the gates of test_gpu_train.py::test_trainer_gradients_vs_autograd (two blocks: the tail is half the model)."""
    _, _, _, ref_loss, ref_logits, _ = _problem(name, R)
    tr, logits, loss, err = _tail_errors(name, R, **kw)
    assert rel_l2(logits.cpu(), ref_logits) < 2e-2
    assert abs(float(loss[0]) - float(ref_loss)) < 2e-2 * abs(float(ref_loss))
    bad = {k: e for k, e in err.items() if e > 2e-2}
    assert not bad, bad


def test_cls_tail_trainer_vit_b16_vs_autograd(yv):
    """ViT-B/16 at R = 4 with the gates of test_gpu_configs.py::test_config2_vit_b16_trainer_vs_autograd."""
    from test_gpu_configs import GRAD_TOL, GRAD_TOL_MEDIAN
    name, R = "vit_base_patch16_224", 4
    _, _, _, ref_loss, ref_logits, _ = _problem(name, R)
    tr, logits, loss, err = _tail_errors(name, R)
    assert rel_l2(logits.cpu(), ref_logits) < 2e-2
    assert abs(float(loss[0]) - float(ref_loss)) < 2e-2 * abs(float(ref_loss))
    worst = sorted(err.items(), key=lambda kv: -kv[1])
    vals = sorted(err.values())
    print("ViT-B/16 cls_tail gradient rel-L2 vs fp32 autograd: median %.4f, max %.4f (%s)" % (vals[len(vals) // 2], worst[0][1], worst[0][0]))
    assert len(err) == 12 * 12 + 8 + 4
    assert worst[0][1] < GRAD_TOL, worst[:6]
    assert vals[len(vals) // 2] < GRAD_TOL_MEDIAN


@pytest.mark.parametrize("name,R", [("vit_tiny_test", 33), ("vit_tiny8_test", 2)])
def test_cls_tail_mx_trainer_gradients(yv, name, R):
    """The fp32 gates of test_gpu_mx_train.py::test_mx_trainer_gradients (the emulation gate does not apply: the emulation quantises
    the last block's small products, the trainer runs them in bf16)."""
    ref_loss = _problem(name, R)[3]
    tr, logits, loss, err = _tail_errors(name, R, dtype="mxfp8")
    assert tr.dtype == "mxfp8"
    assert abs(float(loss[0]) - float(ref_loss)) < 3e-2 * abs(float(ref_loss))
    assert max(err.values()) <= 0.12, sorted(err.items(), key=lambda kv: -kv[1])[:3]


# ------------------------------------------------------------------------------------------------ 3. trainer structure
@pytest.mark.parametrize("dtype", ["bf16", "mxfp8"])
def test_cls_tail_trainer_launchers(yv, monkeypatch, dtype):
    """One backward with L = 2: the full attention backward runs L - 1 times and the cls backward once; three of the last block's four
    weight gradients run over _r64(R) token rows (in the MX recipe the fourth, qkv, is an MX product and not a wgrad call)."""
    from yvhip import training
    name, R = "vit_tiny_test", 3
    calls = {"attention_bwd": 0, "attention_bwd_long": 0, "attention_cls_bwd": 0, "attention_cls_train": 0, "attention_train": 0}
    wg = []

    def counting(fname):
        real = getattr(training, fname)

        def wrapper(*a, **k):
            calls[fname] += 1
            return real(*a, **k)
        return wrapper

    for fname in calls:
        monkeypatch.setattr(training, fname, counting(fname))
    real_wgrad = training.wgrad

    def wgrad(dy, x, dw, T=None):
        wg.append((dw.data_ptr(), dy.shape[0] if T is None else T))
        return real_wgrad(dy, x, dw, T=T)

    monkeypatch.setattr(training, "wgrad", wgrad)
    tr = _train(name, R, cls_tail=True, dtype=dtype)[0]
    L, N = tr.L, tr.N
    assert L == 2 and N <= 224
    assert calls["attention_bwd"] + calls["attention_bwd_long"] == L - 1 and calls["attention_cls_bwd"] == 1
    assert calls["attention_train"] == L - 1 and calls["attention_cls_train"] == 1
    last = {tr.g(f"model.blocks.{L - 1}.{w}").data_ptr(): w for w in training.BLOCK_LINEARS}
    rows = {last[p]: T for p, T in wg if p in last}
    small = sorted(w for w, T in rows.items() if T == _r64(R))
    assert small == ["attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"]
    if dtype == "bf16":
        assert rows["attn.qkv.weight"] == _r64(R * N) and len(rows) == 4
        first = {tr.g(f"model.blocks.0.{w}").data_ptr() for w in training.BLOCK_LINEARS}
        assert [T for p, T in wg if p in first] == [_r64(R * N)] * 4                      # the other block: every row, as before
    else:
        assert len(rows) == 3


@pytest.mark.parametrize("dtype", ["bf16", "mxfp8"])
def test_cls_tail_trainer_is_deterministic(yv, dtype):
    from yvhip.training import VitTrainer
    name, R = "vit_tiny_test", 5
    sd = _problem(name, 3)[0]
    g = torch.Generator().manual_seed(12)
    pm = bf(torch.rand(R * 196, 768, generator=g) * 2 - 1).to(DEV)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(DEV)
    tr = VitTrainer(sd, name, 5, cls_tail=True, dtype=dtype)
    runs = []
    for _ in range(2):
        logits = tr.forward(pm, R).clone()
        loss = tr.backward(pm, labels, R).clone()
        torch.cuda.synchronize()
        runs.append((logits, loss, tr.grad_dict()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k, v in runs[0][2].items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(v, runs[1][2][k]), k


def test_cls_tail_trainer_full_step(yv):
    from yvhip.training import VitTrainer
    name, R = "vit_tiny_test", 8
    sd = _problem(name, 3)[0]
    g = torch.Generator().manual_seed(13)
    pm = bf(torch.rand(R * 196, 768, generator=g) * 2 - 1).to(DEV)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(DEV)
    tr = VitTrainer(sd, name, 5, cls_tail=True)
    losses = [float(tr.step(pm, labels, 0.004)[0][0]) for _ in range(2)]
    torch.cuda.synchronize()
    print(f"cls_tail step losses: {losses}")
    assert math.isfinite(losses[0]) and losses[1] < losses[0]
    for k, v in tr.state_dict().items():
        assert bool(torch.isfinite(v).all()), k


def test_cls_tail_default_and_environment(yv, monkeypatch):
    from yvhip.training import VitTrainer
    name = "vit_tiny_test"
    sd = _problem(name, 3)[0]
    for var in ("YV_VIT_TRAIN_CLS_TAIL", "YV_VIT_LONG_ATTN", "YV_VIT_LONG_ATTN_BWD"):
        monkeypatch.delenv(var, raising=False)
    tr = VitTrainer(sd, name, 5)
    assert tr.cls_tail is False and tr.long_attn is False and tr.long_attn_bwd is False       # default off
    tr = VitTrainer(sd, name, 5, cls_tail=True)                                                # independent flags
    assert tr.cls_tail is True and tr.long_attn is False and tr.long_attn_bwd is False
    tr = VitTrainer(sd, name, 5, long_attn=True, long_attn_bwd=True)
    assert tr.cls_tail is False
    monkeypatch.setenv("YV_VIT_LONG_ATTN", "1")
    monkeypatch.setenv("YV_VIT_LONG_ATTN_BWD", "1")
    assert VitTrainer(sd, name, 5).cls_tail is False
    monkeypatch.setenv("YV_VIT_TRAIN_CLS_TAIL", "1")
    tr = VitTrainer(sd, name, 5, long_attn=False)
    assert tr.cls_tail is True and tr.long_attn is False and tr.long_attn_bwd is True
    assert VitTrainer(sd, name, 5, cls_tail=False).cls_tail is False                           # an argument overrides it
    assert VitTrainer(sd, name, 5, cls_tail=True, dtype="mxfp8").dtype == "mxfp8"


def test_cls_tail_off_is_the_default_trainer(yv, monkeypatch):
    monkeypatch.delenv("YV_VIT_TRAIN_CLS_TAIL", raising=False)
    name, R = "vit_tiny_test", 3
    _, logits, loss, ref = _train(name, R)
    tr, logits2, loss2, got = _train(name, R, cls_tail=False)
    assert tr.cls_tail is False and "tail" not in tr._buffers(R)
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2)
    for k, v in ref.items():
        assert torch.equal(got[k], v), k
