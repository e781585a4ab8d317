"""GPU checks of the one-launch attention backward (yv_attention_bwd_short): bit equality with yv_attention_bwd for every
NT = ceil(N / 32) from 1 to 7 (a last 32-row group with one live row, a full one, the model's 197 tokens, several crops and
heads, an odd head count), fp32 autograd under the gates of tests/test_gpu_train.py::test_attention_bwd, isolation of crops and of
the memory past the live rows, independence of a crop's bits from the launch, and VitTrainer(short_attn_bwd=True) against the
default trainer bit for bit.  The bit contract holds because both files walk a row's reduction in ascending 16-row MFMA steps
inside one wave with the same element-wise expressions, and rows past N contribute exact zeros.  A workgroup takes one
(crop, head) item whatever the shape, so there is no items-per-workgroup seam to aim at."""
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


def make_inputs(yv, R, N, H, seed, fwd="attention_train"):
    """qkv = bf16(randn * 1.5), dout = bf16(randn), out and lse from the named forward: all on the device."""
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    qkv = bf(torch.randn(R * N, 3 * D, generator=g) * 1.5).to(DEV)
    dout = bf(torch.randn(R * N, D, generator=g)).to(DEV)
    out = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(R * H * N, device=DEV)
    if fwd == "attention_long":
        yv.attention_long(qkv, R, N, H, out, lse=lse)
    else:
        yv.attention_train(qkv, R, N, H, out, lse)
    return qkv, out, dout, lse


def run_bwd(fn, qkv, out, dout, lse, R, N, H):
    """-> (dqkv with 64 extra rows, delta_ws with 64 extra floats), both pre-filled with 1.5"""
    dqkv = torch.full((R * N + 64, 3 * H * 64), 1.5, dtype=torch.bfloat16, device=DEV)
    dws = torch.full((R * H * N + 64,), 1.5, device=DEV)
    fn(qkv, out, dout, lse, R, N, H, dqkv, dws)
    torch.cuda.synchronize()
    return dqkv, dws


# ------------------------------------------------------------------------------------------------ 1. bits
SHAPES = [(1, 1, 1), (2, 5, 2), (1, 32, 1), (2, 33, 1), (1, 64, 2), (1, 65, 1), (1, 97, 3), (2, 129, 1), (1, 161, 1), (1, 192, 1),
          (2, 193, 2), (3, 197, 2), (1, 224, 1)]
CASES = [(*s, "attention_train") for s in SHAPES] + [(2, 197, 2, "attention_long")]


@pytest.mark.parametrize("R,N,H,fwd", CASES)
def test_attention_bwd_short_bits(yv, R, N, H, fwd):
    ins = make_inputs(yv, R, N, H, R * 7 + N, fwd)
    ref, ref_d = run_bwd(yv.attention_bwd, *ins, R, N, H)
    got, got_d = run_bwd(yv.attention_bwd_short, *ins, R, N, H)
    rows, fl = R * N, R * H * N
    assert bool(torch.isfinite(ref[:rows].float()).all()) and bool(torch.isfinite(ref_d[:fl]).all())
    assert bool(torch.isfinite(got[:rows].float()).all()) and bool(torch.isfinite(got_d[:fl]).all())
    assert torch.equal(got_d[:fl], ref_d[:fl])
    D = H * 64
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert torch.equal(got[:rows, sl], ref[:rows, sl]), name
    assert bool((got[rows:] == 1.5).all()) and bool((got_d[fl:] == 1.5).all())


def test_attention_bwd_short_refuses_more_than_224_tokens(yv):
    R, N, H = 1, 225, 1
    ins = make_inputs(yv, R, N, H, 5)
    with pytest.raises(yv.YvError):
        run_bwd(yv.attention_bwd_short, *ins, R, N, H)


# ------------------------------------------------------------------------------------------------ 2. fp32 autograd
@pytest.mark.parametrize("R,N,H", [(2, 197, 2), (2, 33, 1)])
def test_attention_bwd_short_vs_autograd(yv, R, N, H):
    """Body and gates of test_gpu_train.py::test_attention_bwd."""
    g = torch.Generator().manual_seed(R + N)
    D = H * 64
    qkv = bf(torch.randn(R * N, 3 * D, generator=g))
    do = bf(torch.randn(R * N, D, generator=g))
    t = qkv.float().clone().requires_grad_(True)
    tt = t.view(R, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    att = ((tt[0] * 0.125) @ tt[1].transpose(-2, -1)).softmax(-1)
    ref_o = (att @ tt[2]).transpose(1, 2).reshape(R * N, D)
    ref_o.backward(do.float())
    out = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV); lse = torch.zeros(R * H * N, device=DEV)
    yv.attention_train(qkv.to(DEV), R, N, H, out, lse)
    assert rel_l2(out.cpu().float(), ref_o.detach()) < 8e-3
    dqkv = torch.zeros(R * N, 3 * D, dtype=torch.bfloat16, device=DEV); dws = torch.zeros(R * H * N, device=DEV)
    yv.attention_bwd_short(qkv.to(DEV), out, do.to(DEV), lse, R, N, H, dqkv, dws)
    got = dqkv.cpu().float()
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert rel_l2(got[:, sl], t.grad[:, sl]) < 2e-2, name


# ------------------------------------------------------------------------------------------------ 3. isolation
def crop_of(ins, r, N, H):
    qkv, out, dout, lse = ins
    return (qkv[r * N:(r + 1) * N].contiguous(), out[r * N:(r + 1) * N].contiguous(), dout[r * N:(r + 1) * N].contiguous(),
            lse[r * H * N:(r + 1) * H * N].contiguous())


@pytest.mark.parametrize("bad", [0, 1])
def test_attention_bwd_short_no_leak_across_crops(yv, bad):
    R, N, H = 2, 197, 2
    ins = make_inputs(yv, R, N, H, 31)
    good = 1 - bad
    alone, alone_d = run_bwd(yv.attention_bwd_short, *crop_of(ins, good, N, H), 1, N, H)
    assert bool(torch.isfinite(alone[:N].float()).all()) and bool(torch.isfinite(alone_d[:H * N]).all())
    qkv, out, dout, lse = ins
    for t in (qkv, out, dout):
        t[bad * N:(bad + 1) * N] = float("nan")
    lse[bad * H * N:(bad + 1) * H * N] = float("nan")
    got, got_d = run_bwd(yv.attention_bwd_short, qkv, out, dout, lse, R, N, H)
    assert torch.equal(got[good * N:(good + 1) * N], alone[:N])
    assert torch.equal(got_d[good * H * N:(good + 1) * H * N], alone_d[:H * N])


@pytest.mark.parametrize("N", [33, 197])
def test_attention_bwd_short_crop_bits_do_not_depend_on_the_launch(yv, N):
    R, H = 3, 2
    ins = make_inputs(yv, R, N, H, N)
    whole, whole_d = run_bwd(yv.attention_bwd_short, *ins, R, N, H)
    for r in range(R):
        alone, alone_d = run_bwd(yv.attention_bwd_short, *crop_of(ins, r, N, H), 1, N, H)
        assert torch.equal(whole[r * N:(r + 1) * N], alone[:N]), r
        assert torch.equal(whole_d[r * H * N:(r + 1) * H * N], alone_d[:H * N]), r


# ------------------------------------------------------------------------------------------------ 4. trainer
@functools.lru_cache(maxsize=None)
def _problem(name):
    from yvhip import engines
    P = engines.vit_cfg(name)[0]
    R = 2
    sd = engines.init_vit_wrapper_state(name, 5, 21)
    g = torch.Generator().manual_seed(R)
    pm = bf(torch.rand(R * (224 // P) ** 2, 3 * P * P, generator=g) * 2 - 1).to(DEV)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(DEV)
    return sd, pm, labels, R


def _train(name, **kw):
    """One forward + backward of a fresh trainer on the shared problem -> (trainer, logits, loss, gradients)."""
    from yvhip.training import VitTrainer
    sd, pm, labels, R = _problem(name)
    tr = VitTrainer(sd, name, 5, **kw)
    logits = tr.forward(pm, R).clone()
    loss = tr.backward(pm, labels, R).clone()
    torch.cuda.synchronize()
    return tr, logits, loss, tr.grad_dict()


@functools.lru_cache(maxsize=None)
def _default_run(dtype, cls_tail):
    return _train("vit_tiny_test", dtype=dtype, cls_tail=cls_tail, short_attn_bwd=False)[1:]


@pytest.mark.parametrize("dtype,cls_tail", [("bf16", False), ("mxfp8", False), ("bf16", True)])
def test_trainer_short_attn_bwd_equals_default(yv, dtype, cls_tail):
    ref_logits, ref_loss, ref = _default_run(dtype, cls_tail)
    tr, logits, loss, got = _train("vit_tiny_test", dtype=dtype, cls_tail=cls_tail, short_attn_bwd=True)
    assert tr.short_attn_bwd and tr.N == 197 and tr.cls_tail is cls_tail
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss).all())
    assert torch.equal(logits, ref_logits) and torch.equal(loss, ref_loss)
    assert sorted(got) == sorted(ref)
    for k, v in ref.items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(got[k], v), k


def test_trainer_short_attn_bwd_launchers(yv, monkeypatch):
    from yvhip import training
    calls = {"attention_bwd_short": 0, "attention_bwd": 0, "attention_bwd_long": 0, "attention_cls_bwd": 0}

    def counting(fname):
        real = getattr(training, fname)

        def wrapper(*a, **k):
            calls[fname] += 1
            return real(*a, **k)
        return wrapper

    for fname in calls:
        monkeypatch.setattr(training, fname, counting(fname))

    def run(name, **kw):
        for k in calls:
            calls[k] = 0
        tr = _train(name, **kw)[0]
        return tr.L, calls["attention_bwd_short"], calls["attention_bwd"], calls["attention_bwd_long"], calls["attention_cls_bwd"]

    for dtype in ("bf16", "mxfp8"):
        L, new, old, long_, cls = run("vit_tiny_test", dtype=dtype, short_attn_bwd=True)
        assert L > 0 and (new, old, long_, cls) == (L, 0, 0, 0), dtype
        L, new, old, long_, cls = run("vit_tiny_test", dtype=dtype, short_attn_bwd=False)
        assert (new, old, long_, cls) == (0, L, 0, 0), dtype
    L, new, old, long_, cls = run("vit_tiny_test", cls_tail=True, short_attn_bwd=True)
    assert L > 1 and (new, old, long_, cls) == (L - 1, 0, 0, 1)
    L, new, old, long_, cls = run("vit_tiny_test", cls_tail=True, short_attn_bwd=False)
    assert (new, old, long_, cls) == (0, L - 1, 0, 1)
    L, new, old, long_, cls = run("vit_tiny8_test", short_attn_bwd=True)          # 785 tokens: accepted, not effective
    assert (new, old, long_, cls) == (0, L, 0, 0)
    L, new, old, long_, cls = run("vit_tiny8_test", short_attn_bwd=True, long_attn_bwd=True)
    assert (new, old, long_, cls) == (0, 0, L, 0)


def test_trainer_short_attn_bwd_default_and_environment(yv, monkeypatch):
    from yvhip.training import VitTrainer
    sd = _problem("vit_tiny_test")[0]
    monkeypatch.delenv("YV_VIT_SHORT_ATTN_BWD", raising=False)
    monkeypatch.delenv("YV_VIT_LONG_ATTN_BWD", raising=False)
    tr = VitTrainer(sd, "vit_tiny_test", 5)
    assert tr.short_attn_bwd is False and tr.long_attn_bwd is False
    assert VitTrainer(sd, "vit_tiny_test", 5, long_attn_bwd=True).short_attn_bwd is False      # independent flags
    assert VitTrainer(sd, "vit_tiny_test", 5, short_attn_bwd=True).long_attn_bwd is False
    monkeypatch.setenv("YV_VIT_SHORT_ATTN_BWD", "1")
    assert VitTrainer(sd, "vit_tiny_test", 5).short_attn_bwd is True
    assert VitTrainer(sd, "vit_tiny_test", 5).long_attn_bwd is False
    assert VitTrainer(sd, "vit_tiny_test", 5, short_attn_bwd=False).short_attn_bwd is False    # an argument overrides it
