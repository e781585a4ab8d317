"""GPU tests of global-norm gradient clipping: yv_grad_clip_record (csrc/train.hip) against the exact integer
sum, the fp64 sum and the numpy statement of the record (tests/grad_clip_reference.py); yv_sgd_step_rec / yv_optim_step_rec against
the plain steps, bit for bit, and their no-op on a record that is not finite; the pair against torch's clip_grad_norm_ + optimiser;
YoloTrainer(clip_grad=) and utils.trainYolo.train(clip_grad=).

Every buffer is longer than the call is told: inputs past n are NaN, outputs past n a sentinel that must stay.  The workspace is filled
with 0xFF bytes (NaN as f64) before every call, so a partial that is stale or was never written shows in the sum."""
import math

import numpy as np
import pytest
import torch

import grad_clip_reference as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, SENTINEL, PAD = float("nan"), -24576.0, 8
f32 = np.float32
# the reduction's own constants (csrc/train.hip): test_constants_are_the_kernels ties them to what the library says
CLIP_BLOCK_ELEMS = 256 * 4 * 4                            # CLIP_THREADS * CLIP_UNROLL * 4: one workgroup's share of one trip
CLIP_MAX_BLOCKS = 1024                                    # the grid's cap
CLIP_TRIP_ELEMS = CLIP_MAX_BLOCKS * CLIP_BLOCK_ELEMS      # what one full grid covers in one trip
LARGE_NS = (CLIP_TRIP_ELEMS - 1, CLIP_TRIP_ELEMS + 3, 2 * CLIP_TRIP_ELEMS + 5)
SGD_GRID_ELEMS, OPTIM_GRID_ELEMS = 2048 * 256 * 4, 4096 * 256          # one trip of sgd_kernel / optim_kernel


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _padded(live, fill=NAN, dtype=torch.float32):
    """device buffer of live.numel() + PAD elements: `live` in front, `fill` behind"""
    buf = torch.full((live.numel() + PAD,), fill, dtype=dtype, device=DEV)
    buf[:live.numel()] = live.reshape(-1).to(DEV)
    return buf


class Clip:
    """One call of grad_clip_record on a gradient with NaN behind it, a workspace of 0xFF bytes with guard bytes behind it, a record
    with sentinels behind it and a counter that starts at `count0`."""
    GUARD = 64

    def __init__(self, yv, g_host, count0=5):
        self.yv, self.n = yv, g_host.numel()
        self.gbuf = _padded(g_host)
        self.need = yv.grad_clip_ws_bytes(self.n)
        self.ws = torch.empty(self.need + self.GUARD, dtype=torch.uint8, device=DEV)
        self.recbuf = torch.full((4 + 4,), SENTINEL, device=DEV)
        self.skipped = torch.full((1 + 3,), count0, dtype=torch.int32, device=DEV)
        self.count0 = count0

    @property
    def rec(self):
        return self.recbuf[:4]

    def run(self, grad_scale=1.0, max_norm=10.0):
        """-> (the record as four numpy f32, how far the counter moved)"""
        before = int(self.skipped[0])
        self.ws.fill_(0xFF)
        self.yv.grad_clip_record(self.gbuf[:self.n], grad_scale, max_norm, self.ws[:self.need], self.rec, self.skipped[:1])
        torch.cuda.synchronize()
        assert bool((self.ws[self.need:] == 0xFF).all()), "workspace written past yv_grad_clip_ws_bytes"
        assert bool((self.recbuf[4:] == SENTINEL).all()) and self.skipped[1:].tolist() == [self.count0] * 3
        return self.rec.cpu().numpy().copy(), int(self.skipped[0]) - before


def _record_equals_statement(rec, grad_scale, max_norm):
    """rec[1..3] are the numpy statement applied to rec[0], bit for bit (a NaN norm: NaN, whatever its payload); -> the skip flag"""
    S, N, c, s, skip = gc.record(rec[0], grad_scale, max_norm)
    want = np.array([S, N, c, s], f32)
    if skip and np.isnan(N):
        assert np.isnan(rec[1]) and rec[2:].tobytes() == want[2:].tobytes(), (rec, want)
    else:
        assert rec[1:].tobytes() == want[1:].tobytes(), (rec, want)
    return skip


# ------------------------------------------------------------------------------------------------ the sum
_INTS = {}


def _int_case(n):
    """n values of {-2, ..., 2} (zeros and ones the most, so that the largest n stays below 2^24) and their integer sum of squares"""
    if n not in _INTS:
        rng = np.random.default_rng(n)
        x = rng.choice(np.array([-2, -1, 0, 1, 2], np.int64), size=n, p=[0.05, 0.2, 0.5, 0.2, 0.05])
        if n >= 5:
            x[:5] = [-2, -1, 0, 1, 2]                                 # every value is there, the tail element included
            x[-1] = 2
        else:
            x[:] = [2, -1, 1, -2][:n]
        _INTS[n] = (torch.from_numpy(x.astype(np.float32)), int((x * x).sum()))
    return _INTS[n]


def test_constants_are_the_kernels(yv):
    assert yv.grad_clip_ws_bytes(CLIP_BLOCK_ELEMS) == 8 and yv.grad_clip_ws_bytes(CLIP_BLOCK_ELEMS + 1) == 16
    assert yv.grad_clip_ws_bytes(CLIP_TRIP_ELEMS - CLIP_BLOCK_ELEMS) == 8 * (CLIP_MAX_BLOCKS - 1)
    assert yv.grad_clip_ws_bytes(CLIP_TRIP_ELEMS) == yv.grad_clip_ws_bytes(1 << 40) == 8 * CLIP_MAX_BLOCKS


@pytest.mark.parametrize("n", (1, 3, 4, 255, 257, CLIP_BLOCK_ELEMS - 1, CLIP_BLOCK_ELEMS + 1) + LARGE_NS)
def test_sum_of_small_integers_is_exact(yv, n):
    """Every partial sum is an integer below 2^24, exact in f32 and in f64 in any order: rec[0] is that integer, bit for bit."""
    g, total = _int_case(n)
    assert 0 < total < 1 << 24
    rec, moved = Clip(yv, g).run()
    print(f"n={n}: sum of squares {total}, rec[0] {rec[0]}")
    assert rec[0].tobytes() == f32(total).tobytes() and moved == 0
    assert not _record_equals_statement(rec, 1.0, 10.0)


_RANDOM = {}


def _random_case(n):
    if n not in _RANDOM:
        g = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000)) * 0.01
        _RANDOM[n] = (g, gc.sum_squares_f64(g.numpy()))
    return _RANDOM[n]


@pytest.mark.parametrize("n", LARGE_NS)
def test_sum_of_random_data_within_one_ulp_and_repeatable(yv, n):
    """Squares are exact in f64 and n * 2^-53 is far below half an f32 ulp (2^-25) for n < 2^26, so the kernel's f64 sum and the
    reference's round to the same f32 or to neighbours: one ulp.  A second call on the same input gives the same bits."""
    g, ref = _random_case(n)
    call = Clip(yv, g)
    rec, _ = call.run()
    d = gc.ulps(rec[0], f32(ref))
    print(f"n={n}: rec[0] {rec[0]!r}, fp64 {ref!r}, {d} ulp")
    assert np.isfinite(rec[0]) and d <= 1
    again, _ = call.run()
    assert again.tobytes() == rec.tobytes()
    assert not _record_equals_statement(rec, 1.0, 10.0)


# ------------------------------------------------------------------------------------------------ the record
def _g(n, scale, seed=11):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("name,scale,grad_scale,max_norm,clips", [
    ("above", 1.0, 1.0, 10.0, True),                                  # norm about 64
    ("below", 0.01, 0.7, 10.0, False),                                # norm about 0.64 * 0.7: c == 1.0 and s == grad_scale exactly
    ("third", 1.0, 1.0 / 3.0, 10.0, True),
    ("third_below", 0.1, 1.0 / 3.0, 10.0, False),
    ("never", 1.0, 1.0, float("inf"), False),
    ("negative_scale", 1.0, -0.5, 10.0, True),
])
def test_record_arithmetic(yv, name, scale, grad_scale, max_norm, clips):
    """rec[1..3] are the numpy statement applied to the kernel's own rec[0], bit for bit; the counter stays."""
    rec, moved = Clip(yv, _g(4099, scale)).run(grad_scale, max_norm)
    print(f"{name}: {rec}")
    assert not _record_equals_statement(rec, grad_scale, max_norm) and moved == 0
    assert (rec[2] < 1.0) == clips
    if not clips:
        assert rec[2].tobytes() == f32(1.0).tobytes() and rec[3].tobytes() == f32(grad_scale).tobytes()


@pytest.mark.parametrize("name", ["one_nan", "overflow", "one_inf"])
def test_record_of_a_gradient_that_is_not_finite(yv, name):
    """One NaN element, or elements of 1e20 whose squares pass f32 (the f64 sum holds them: S rounds to inf): the norm is not finite,
    coefficient and scale are 0, the counter rises by exactly one per call."""
    g = _g(4099, 1.0)
    if name == "one_nan":
        g[2048] = NAN
    elif name == "one_inf":
        g[4098] = float("inf")
    else:
        g[::7] = 1e20
    call = Clip(yv, g)
    for _ in range(2):
        rec, moved = call.run()
        assert _record_equals_statement(rec, 1.0, 10.0) and moved == 1
        assert not np.isfinite(rec[1]) and rec[2] == 0 and rec[3] == 0
    assert math.isnan(rec[0]) if name == "one_nan" else np.isinf(rec[0])


def test_record_without_a_counter(yv):
    g = _g(259, 1.0)
    g[0] = NAN
    gbuf, rec = _padded(g), torch.zeros(4, device=DEV)
    ws = torch.full((yv.grad_clip_ws_bytes(259),), 0xFF, dtype=torch.uint8, device=DEV)
    yv.grad_clip_record(gbuf[:259], 1.0, 10.0, ws, rec)
    torch.cuda.synchronize()
    assert math.isnan(float(rec[1])) and rec[2:].tolist() == [0.0, 0.0]
    with pytest.raises(yv.YvError):
        yv.grad_clip_record(gbuf[:259], 1.0, -1.0, ws, rec)
    with pytest.raises(yv.YvError):
        yv.grad_clip_record(gbuf[:259], 1.0, 10.0, ws[:-1], rec)
    with pytest.raises(yv.YvError, match="grad_scale"):
        yv.sgd_step(gbuf[:256], gbuf[:256], gbuf[:256], 1e-3, grad_scale=0.5, scale_rec=rec)


# ------------------------------------------------------------------------------------------------ the steps
KINDS = ("sgd", "sgd_nesterov", "adamw")


def _step(yv, kind, p, g, m, v, lr, t, mirror, **scale):
    if kind == "sgd":
        yv.sgd_step(p, g, m, lr, 0.937, 5e-4, t == 1, mirror=mirror, **scale)
    else:
        yv.optim_step(yv.OPT_ADAMW if kind == "adamw" else yv.OPT_SGD_NESTEROV, p, g, m, v, lr, t, beta1=0.9, weight_decay=5e-4,
                      mirror=mirror, **scale)


class _State:
    """p, m, v and the bf16 mirror of n parameters with sentinels behind them; m and v start as NaN (a first step must not read them)"""

    def __init__(self, p0, with_mirror):
        n = self.n = p0.numel()
        self.p, self.m, self.v = _padded(p0, SENTINEL), _padded(torch.full((n,), NAN), SENTINEL), _padded(torch.full((n,), NAN), SENTINEL)
        self.mirror = torch.full((n + PAD,), SENTINEL, dtype=torch.bfloat16, device=DEV) if with_mirror else None

    def buffers(self):
        return [b for b in (self.p, self.m, self.v, self.mirror) if b is not None]

    def step(self, yv, kind, g, lr, t, **scale):
        n = self.n
        _step(yv, kind, self.p[:n], g[:n], self.m[:n], self.v[:n], lr, t, None if self.mirror is None else self.mirror[:n], **scale)


@pytest.mark.parametrize("with_mirror", [True, False])
@pytest.mark.parametrize("n_name", ["3", "4099", "past_the_grid"])
@pytest.mark.parametrize("kind", KINDS)
def test_rec_steps_equal_the_plain_steps(yv, kind, n_name, with_mirror):
    """A first and a later step: scale_rec=rec gives the bits of grad_scale=float(rec[3]) in p, m, v and the mirror, and nothing past
    n is written.  The first record clips (max_norm 1e-3: its scale is no round number), the second does not (max_norm 1e3: its scale
    is grad_scale = 1/3)."""
    n = {"3": 3, "4099": 4099, "past_the_grid": (SGD_GRID_ELEMS if kind == "sgd" else OPTIM_GRID_ELEMS) + 3}[n_name]
    gen = torch.Generator().manual_seed(n % 1000 + len(kind))
    p0 = torch.randn(n, generator=gen)
    a, b = _State(p0, with_mirror), _State(p0, with_mirror)
    for t, (scale, grad_scale, max_norm, lr) in enumerate(((1.0, 1.0, 1e-3, 1e-3), (0.001, 1.0 / 3.0, 1e3, 9.75528e-4)), start=1):
        g = torch.randn(n, generator=gen) * scale
        call = Clip(yv, g)
        rec, _ = call.run(grad_scale, max_norm)
        assert (rec[2] < 1.0) == (t == 1) and np.isfinite(rec[1])
        a.step(yv, kind, call.gbuf, lr, t, scale_rec=call.rec)
        b.step(yv, kind, call.gbuf, lr, t, grad_scale=float(rec[3]))
        torch.cuda.synchronize()
        for x, y in zip(a.buffers(), b.buffers()):
            if kind != "adamw" and x is a.v:
                continue
            assert _same_bits(x, y)
            assert bool((x[n:] == SENTINEL).all()) and bool(torch.isfinite(x[:n].float()).all())
        assert not _same_bits(a.p[:n], p0)
    if kind != "adamw":
        assert bool(torch.isnan(a.v[:n]).all())                       # no second moment: never touched


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_rec_steps_skip_on_a_record_that_is_not_finite(yv, kind, first):
    """p, m, v and the mirror keep their bits; on a first step m / v are NaN before and after (neither read nor written).  The same
    buffers then take an ordinary step, so the launch above was one that would have written."""
    n = OPTIM_GRID_ELEMS + 3 if kind == "adamw" else 4099
    gen = torch.Generator().manual_seed(3)
    st = _State(torch.randn(n, generator=gen), True)
    if not first:
        st.m[:n] = torch.randn(n, generator=gen).to(DEV) * 0.01
        st.v[:n] = torch.rand(n, generator=gen).to(DEV) * 1e-4
    st.mirror[:n] = st.p[:n].to(torch.bfloat16)
    before = [x.clone() for x in st.buffers()]
    g = torch.randn(n, generator=gen)
    bad = g.clone()
    bad[n // 2] = NAN
    call = Clip(yv, bad)
    rec, moved = call.run()
    assert moved == 1 and not np.isfinite(rec[1])
    t = 1 if first else 2
    st.step(yv, kind, call.gbuf, 1e-3, t, scale_rec=call.rec)
    torch.cuda.synchronize()
    for x, y in zip(st.buffers(), before):
        assert _same_bits(x, y)
    good = Clip(yv, g)
    good.run()
    st.step(yv, kind, good.gbuf, 1e-3, t, scale_rec=good.rec)
    torch.cuda.synchronize()
    assert not _same_bits(st.p[:n], before[0][:n]) and bool(torch.isfinite(st.p[:n]).all()) and bool((st.p[n:] == SENTINEL).all())


@pytest.mark.parametrize("kind", ["sgd_nesterov", "adamw"])
def test_clip_and_step_match_torch(yv, kind):
    """Five parameter tensors of unequal size, three steps of torch.nn.utils.clip_grad_norm_ + torch.optim on the CPU against
    grad_clip_record + optim_step(scale_rec=) on the flat buffer; max_norm 10 lies between the norms of the steps (about 3.8, 38,
    7.5), so the second step clips and the others do not.  Parameters: the relative measure and the 1e-5 of
    test_gpu_yolo_train.py::test_optimisers_match_torch plus 4 f32 ulps (4 * 2^-23) for the coefficient, which torch forms from an
    f32 norm.  rec[1] against the fp64 norm: 2 ulps (one for the rounding of S, half of which the root keeps, one for the root)."""
    sizes, max_norm = [1000, 37, 4099, 1, 513], 10.0
    n = sum(sizes)
    gen = torch.Generator().manual_seed(6)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * s for s in (0.05, 0.5, 0.1)]
    lrs = [1e-3, 2e-3, 5e-4]
    params = [torch.nn.Parameter(t.clone()) for t in p0.split(sizes)]
    if kind == "adamw":
        opt = torch.optim.AdamW(params, lr=lrs[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
        code, b1 = yv.OPT_ADAMW, 0.9
    else:
        opt = torch.optim.SGD(params, lr=lrs[0], momentum=0.937, nesterov=True, weight_decay=5e-4)
        code, b1 = yv.OPT_SGD_NESTEROV, 0.937
    p, m, v = _padded(p0, SENTINEL), _padded(torch.zeros(n), SENTINEL), _padded(torch.zeros(n), SENTINEL)
    clipped = []
    for t, (gr, lr) in enumerate(zip(grads, lrs), start=1):
        for grp in opt.param_groups:
            grp["lr"] = lr
        for q, gq in zip(params, gr.split(sizes)):
            q.grad = gq.clone()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        call = Clip(yv, gr)
        rec, moved = call.run(1.0, max_norm)
        yv.optim_step(code, p[:n], call.gbuf[:n], m[:n], v[:n], lr, t, beta1=b1, weight_decay=5e-4, scale_rec=call.rec)
        torch.cuda.synchronize()
        norm64 = math.sqrt(gc.sum_squares_f64(gr.numpy()))
        d = gc.ulps(rec[1], f32(norm64))
        print(f"{kind} step {t}: norm {rec[1]!r} (fp64 {norm64!r}, {d} ulp), coefficient {rec[2]!r}")
        assert d <= 2 and moved == 0
        clipped.append(bool(rec[2] < 1.0))
        ref = torch.cat([q.detach().reshape(-1) for q in params])
        err = float(((p[:n].cpu() - ref).abs() / (ref.abs() + 1e-3)).max())
        print(f"{kind} step {t}: max relative difference {err:.2e}")
        assert err < 1e-5 + 4 * 2.0 ** -23, (t, err)
    assert clipped == [False, True, False]
    assert all(bool((x[n:] == SENTINEL).all()) for x in (p, m, v))


# ------------------------------------------------------------------------------------------------ the trainer
SCALE, NC, SIZE, B, GT = "n", 5, 64, 2, 2               # the trace cases' shape


def _trainer(**kw):
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    return YoloTrainer(init_yolo_train_state(SCALE, NC, seed=3), scale=SCALE, nc=NC, size=SIZE, batch=B, **kw)


@pytest.fixture(scope="module")
def batch(yv):
    g = torch.Generator().manual_seed(21)
    ctr, wh = torch.rand(B, GT, 2, generator=g) * (SIZE - 30) + 15, torch.rand(B, GT, 2, generator=g) * 20 + 8
    return (torch.randint(0, 256, (B, SIZE, SIZE, 3), generator=g, dtype=torch.uint8).to(DEV),
            torch.cat([ctr - wh / 2, ctr + wh / 2], -1).to(DEV),
            torch.randint(0, NC, (B, GT), generator=g, dtype=torch.int32).to(DEV),
            torch.full((B,), GT, dtype=torch.int32).to(DEV))


def _unpacked_sum_squares(tr):
    """fp64 sum of squares of the gradients in their real shapes: no padded channel, class or segment gap takes part"""
    return sum(gc.sum_squares_f64(t.numpy()) for t in tr._unpack(tr.G.cpu()).values())


@pytest.fixture(scope="module")
def measured(yv, batch):
    """Two steps with clip_grad=1e30 (measure, never clip) next to two steps with clipping off; the record and the gradient after
    the first."""
    on, off = _trainer(clip_grad=1e30), _trainer()
    assert off.clip_rec is None and off.clip_ws is None and off.clip_skipped is None
    on.step(*batch)
    off.step(*batch)
    torch.cuda.synchronize()
    rec = on.grad_norm_record.cpu().numpy().copy()
    out = dict(rec=rec, real=_unpacked_sum_squares(on), flat=gc.sum_squares_f64(on.G.cpu().numpy()),
               nonzero=(int((on.G != 0).sum()), sum(int((t != 0).sum()) for t in on._unpack(on.G.cpu()).values())))
    on.step(*batch)
    off.step(*batch)
    torch.cuda.synchronize()
    out.update(on=on, off=off)
    return out


def test_trainer_measuring_changes_nothing(measured):
    on, off = measured["on"], measured["off"]
    assert on.grad_norm_record is on.clip_rec and on.skipped_steps is on.clip_skipped and int(on.skipped_steps[0]) == 0
    for name in ("P", "Mo", "P16", "G"):
        assert _same_bits(getattr(on, name), getattr(off, name)), name
    assert on.step_count == off.step_count == 2


def test_trainer_norm_is_the_norm_of_the_real_gradients(measured):
    """rec[1] against the fp64 norm of the gradients unpacked to the real parameter shapes, 2 ulps: the padded positions of G
    (stem input channels 3 -> 8, the Detect class padding, the gaps between segments) contribute nothing."""
    rec, real, flat = measured["rec"], measured["real"], measured["flat"]
    print(f"rec {rec}, fp64 sum of squares: real shapes {real!r}, all of G {flat!r}; non-zero elements {measured['nonzero']}")
    assert np.isfinite(rec).all() and rec[0] > 0 and rec[2] == 1.0 and rec[3] == 1.0
    assert gc.ulps(rec[1], f32(math.sqrt(real))) <= 2
    assert measured["nonzero"][0] == measured["nonzero"][1] > 0      # all of G, the real shapes: every padded position is zero


def test_trainer_clipped_step_is_the_step_at_the_records_scale(yv, batch, measured):
    """max_norm = half the measured norm: the step clips, and P is that of an unclipped trainer whose optimizer_step was given
    grad_scale = rec[3], bit for bit."""
    on, ref = _trainer(clip_grad=float(measured["rec"][1]) / 2), _trainer()
    on.step(*batch)
    rec = on.grad_norm_record.cpu().numpy()
    assert 0.49 < rec[2] < 0.51 and rec[3] == rec[2] and rec[0].tobytes() == measured["rec"][0].tobytes()
    ref.forward(batch[0])
    ref.loss(*batch[1:])
    ref.backward()
    ref.optimizer_step(grad_scale=float(rec[3]))
    torch.cuda.synchronize()
    for name in ("P", "Mo", "P16"):
        assert _same_bits(getattr(on, name), getattr(ref, name)), name
    assert not _same_bits(on.P, measured["off"].P)


def test_trainer_accumulation_takes_one_record_of_the_accumulated_gradient(yv, batch, monkeypatch):
    from yvhip import yolo_training as yt
    calls = []
    real = yt.grad_clip_record
    monkeypatch.setattr(yt, "grad_clip_record", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    tr = _trainer(clip_grad=10.0)
    tr.step(*batch, accumulate=2)
    torch.cuda.synchronize()
    assert calls == [] and tr.grad_norm_record.tolist() == [0.0] * 4 and tr.step_count == 0
    once = gc.sum_squares_f64(tr.G.cpu().numpy())
    tr.step(*batch, accumulate=2)
    torch.cuda.synchronize()
    assert calls == [1] and tr.step_count == 1
    rec = tr.grad_norm_record.cpu().numpy()
    both = gc.sum_squares_f64(tr.G.cpu().numpy())                     # G holds the accumulated gradient when the optimiser runs
    print(f"rec[0] {rec[0]!r}, fp64: accumulated {both!r}, one batch {once!r}")
    assert gc.ulps(rec[0], f32(both)) <= 1 and both > 2 * once


def test_trainer_skips_a_gradient_that_is_not_finite(yv, batch):
    tr = _trainer(clip_grad=10.0, ema=True)
    tr.step(*batch)
    torch.cuda.synchronize()
    before = {name: getattr(tr, name).clone() for name in ("P", "Mo", "P16")}
    tr.G.fill_(NAN)
    tr.optimizer_step()
    torch.cuda.synchronize()
    for name, t in before.items():
        assert _same_bits(getattr(tr, name), t), name
    assert int(tr.skipped_steps[0]) == 1 and tr.step_count == 2 and tr.ema_updates == 2    # both advance on a skipped step
    assert bool(torch.isfinite(tr.P_ema).all())
    tr.step(*batch)
    torch.cuda.synchronize()
    assert not _same_bits(tr.P, before["P"]) and bool(torch.isfinite(tr.P).all()) and int(tr.skipped_steps[0]) == 1


# ------------------------------------------------------------------------------------------------ the call surface
def _surface_dataset(tmp_path):
    """The dataset recipe of the existing train() tests: generate_annotation XML -> xml2pd -> images/labels tree -> data yaml."""
    import random as _r
    from PIL import Image
    from utils.class_config import xml2pd
    from utils.utils import generate_annotation
    rng = np.random.default_rng(0)
    src = tmp_path / "new"; src.mkdir()
    for i in range(6):
        img = rng.integers(90, 130, (96, 128, 3), dtype=np.uint8)
        x0, y0 = int(rng.integers(8, 60)), int(rng.integers(8, 40))
        img[y0:y0 + 40, x0:x0 + 48] = (220, 40, 40) if i % 2 else (40, 40, 220)
        Image.fromarray(img).save(src / f"im{i}.png")
        generate_annotation("new", f"im{i}.png", f"im{i}.png",
                            [{"sort": i % 2, "xmin": x0, "ymin": y0, "xmax": x0 + 48, "ymax": y0 + 40}], save_dir=str(src) + "/")
    _r.seed(3)
    root = tmp_path / "yolo" / "fold0"
    xml2pd(str(src), yolo_root=str(root))
    (tmp_path / "config.yaml").write_text(f"path: {root}\ntrain: images/train\nval: images/val\nnc: 5\n"
                                          "names: ['good', 'broke', 'lose', 'uncovered', 'circle']\n")
    return str(tmp_path / "config.yaml")


def test_train_reports_the_norm_per_epoch(yv, tmp_path, monkeypatch):
    import utils.trainYolo as ty
    monkeypatch.delenv("YV_YOLO_CLIP_GRAD", raising=False)
    data = _surface_dataset(tmp_path)
    res = ty.train(epochs=1, batch=2, data=data, size=128, save=str(tmp_path / "w" / "clip.pth"), log=lambda s: None, clip_grad=10.0)
    assert res["clip_grad"] == 10.0 and len(res["epochs"]) == 1
    for row in res["epochs"]:
        print(row)
        assert all(k in row for k in ("grad_norm", "clipped", "skipped"))
        assert math.isfinite(row["grad_norm"]) and row["grad_norm"] > 0
        assert isinstance(row["clipped"], int) and isinstance(row["skipped"], int)
        assert 0 <= row["clipped"] <= row["steps"] and row["skipped"] == 0 and math.isfinite(row["loss"])
    res = ty.train(epochs=1, batch=2, data=data, size=128, save=str(tmp_path / "w" / "plain.pth"), log=lambda s: None)
    assert res["clip_grad"] is None
    assert not any(k in row for row in res["epochs"] for k in ("grad_norm", "clipped", "skipped"))
