"""The narrow-output weight-gradient tiles (gemm_tn_narrow_kernel: 64 / 32 (n) x 256 (k), yv_wgrad_tiled, yv_wgrad_conv3_tiled,
YoloTrainer(narrow_wgrad=True)) on the GPU.  Small-integer operands make every sum exact, so those results must EQUAL the fp64
product whatever the tile and the number of token slices; on random operands a narrow tile must give the 128 x 128 tile's bits
for an equal slice count, and stay inside the f32 summation bound under the default slice rule."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, KS, TS = (8, 24, 32, 40, 64, 72, 80), (8, 64, 72, 264, 576), (64, 128, 192, 1088)
TMAX, NMAX, KMAX, XOFF, WOFF, SENT = 1088, 80, 576, 8, 8, -77.0


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@contextlib.contextmanager
def options(yv, **kw):
    old = {k: yv.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            yv.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def _operands(kind):
    """dY inside a wider buffer (row stride 96 > N), X at column XOFF of a wider buffer; integers in [-2, 2] or N(0, 1)."""
    g = torch.Generator().manual_seed(7)
    if kind == "int":
        yb = torch.randint(-2, 3, (TMAX, NMAX + 16), generator=g).float()
        xb = torch.randint(-2, 3, (TMAX, KMAX + 16), generator=g).float()
    else:
        yb, xb = torch.randn(TMAX, NMAX + 16, generator=g), torch.randn(TMAX, KMAX + 16, generator=g)
    return yb.to(torch.bfloat16).to(DEV), xb.to(torch.bfloat16).to(DEV)


@pytest.fixture(scope="module")
def ints():
    """Integer operands and, per T, the fp64 product of the widest case (every case is a corner of it); read-only."""
    yb, xb = _operands("int")
    ref = {T: yb[:T, :NMAX].double().t() @ xb[:T, XOFF:XOFF + KMAX].double() for T in TS}
    return yb, xb, ref


@pytest.fixture(scope="module")
def normals():
    yb, xb = _operands("normal")
    N, K = 72, 576
    y, x = yb[:, :N].double(), xb[:, XOFF:XOFF + K].double()
    return yb, xb, y.t() @ x, y.abs().t() @ x.abs()


def _launch(yv, yb, xb, T, N, K, tile_n):
    """wgrad on the slices; returns (dW region, the wider sentinel-filled tensor it lives in)."""
    wb = torch.full((NMAX + 8, KMAX + 24), SENT, device=DEV)
    yv.wgrad(yb[:T, :N], xb[:T, XOFF:XOFF + K], wb[:N, WOFF:WOFF + K], tile_n=tile_n)
    return wb[:N, WOFF:WOFF + K], wb


def _untouched(wb, N, K):
    c = wb.clone()
    c[:N, WOFF:WOFF + K] = SENT
    return bool((c == SENT).all())


@pytest.mark.parametrize("tile_n", [32, 64, 0])
@pytest.mark.parametrize("T", TS)
def test_wgrad_tiled_exact(yv, ints, T, tile_n):
    """Exact sums: dW must equal the fp64 product for every (N, K), no slice (T = 64: one tile, no prefetch; 128; 192: an odd
    tile count) or two slices of 8 and 9 tiles (T = 1088 with the stream's workspace), and nothing outside [N, K] is written."""
    yb, xb, ref = ints
    for N in NS:
        for K in KS:
            r = yv.wgrad_route(T, N, K, tile_n)
            assert r.slices == (2 if T == 1088 else 1), (T, N, K, r)            # the split path and the no-split path are both reached
            if tile_n:
                assert r.tile_n == tile_n and r.tile_k == 256
            elif N in (40, 64):                # 64 wide, unless that launches fewer workgroups than 128 x 128 tiles (K > 128)
                assert r.tile_n == (64 if K <= 128 else 128), (T, N, K, r)
            else:
                assert r.tile_n == 32 and r.tile_k == 256
            dw, wb = _launch(yv, yb, xb, T, N, K, tile_n)
            assert torch.equal(dw.double(), ref[T][:N, :K]), (T, N, K, tile_n)
            assert _untouched(wb, N, K), (T, N, K, tile_n)


def test_wgrad_tile_128_and_none_are_the_old_entry(yv, ints):
    yb, xb, ref = ints
    for T, N, K in ((1088, 72, 264), (192, 40, 576)):
        a, _ = _launch(yv, yb, xb, T, N, K, None)
        b, wb = _launch(yv, yb, xb, T, N, K, 128)
        assert torch.equal(a, b) and torch.equal(a.double(), ref[T][:N, :K]) and _untouched(wb, N, K)
    with pytest.raises(yv.YvError):
        _launch(yv, yb, xb, 64, 8, 8, 48)


@pytest.mark.parametrize("B,H", [(2, 8), (1, 12)])
def test_wgrad_conv3_tiled_exact(yv, B, H):
    """The 3x3 / stride 1 weight gradient on the zero-padded pixel grid (segment addressing of X), as test_conv_backward runs
    yv_wgrad_conv3: finite junk in the margins and the tail rows of the activation, a zero ring and zero tail in dz.  Equal to
    autograd's conv2d weight gradient (exact sums)."""
    g = torch.Generator().manual_seed(B * 10 + H)
    hp = H + 2
    tpad = B * hp * hp
    tpp, mg = (tpad + 63) // 64 * 64, hp + 1
    T = B * H * H
    for Cin in (8, 16, 32, 64):
        x = torch.randint(-2, 3, (B, Cin, H, H), generator=g).float()
        xd = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
        buf = torch.randint(-3, 4, ((tpp + 2 * mg) * Cin,), generator=g).to(torch.bfloat16).to(DEV)
        xpad = buf[mg * Cin:(mg + tpp) * Cin].view(tpp, Cin)
        yv.view_op(yv.VIEW_PAD, yv.mview(xd), yv.mview(xpad), B, H, H)
        for Cout in (16, 32, 64):
            dz = torch.randint(-2, 3, (B, Cout, H, H), generator=g).float()
            wr = torch.zeros(Cout, Cin, 3, 3, requires_grad=True)
            F.conv2d(x, wr, None, 1, 1).backward(dz)
            want = wr.grad.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).to(DEV)
            dzd = dz.permute(0, 2, 3, 1).reshape(T, Cout).to(torch.bfloat16).to(DEV).contiguous()
            dzp = torch.full((tpp, Cout), 7.0, dtype=torch.bfloat16, device=DEV)
            yv.view_op(yv.VIEW_PAD, yv.mview(dzd), yv.mview(dzp), B, H, H)
            dzp[tpad:].zero_()
            for tile_n in (32, 64, 0):
                wb = torch.full((Cout + 8, 9 * Cin + 8), SENT, device=DEV)
                dw = wb[:Cout, 4:4 + 9 * Cin]
                yv.wgrad_conv3(dzp, xpad, dw, tpp, hp, tile_n=tile_n)
                assert torch.equal(dw, want), (Cin, Cout, tile_n)
                c = wb.clone()
                c[:Cout, 4:4 + 9 * Cin] = SENT
                assert bool((c == SENT).all()), (Cin, Cout, tile_n)


def test_narrow_tiles_give_the_bits_of_the_128_tile(yv, normals):
    """N(0, 1) operands, one slice for every tile ("wgrad_split_cap" = 1, "wgrad_split" = 1): the narrow kernels run the 128 x 128
    kernel's chain of MFMAs on the same values for every dW element, so the results are bit-identical."""
    yb, xb, _, _ = normals
    with options(yv, wgrad_split_cap=1, wgrad_split=1):
        for N, K in ((64, 576), (40, 264)):
            for t in (32, 64, 128):
                assert yv.wgrad_route(TMAX, N, K, t).slices == 1
            base, _ = _launch(yv, yb, xb, TMAX, N, K, 128)
            assert float(base.abs().max()) > 1 and bool((base != base.round()).any())      # not an exact-integer case
            for t in (32, 64):
                got, wb = _launch(yv, yb, xb, TMAX, N, K, t)
                assert torch.equal(got, base), (N, K, t)
                assert _untouched(wb, N, K)
    assert yv.get_option("wgrad_split_cap") == 128 and yv.get_option("wgrad_split") == 0


def test_narrow_tiles_within_the_f32_summation_bound(yv, normals):
    """Default slice rule (two slices at T = 1088), the operands of the bit-identity test.  A product of two bf16 values has at
    most 16 significant bits: exact in f32.  dW[n][k] is therefore a sum of T exactly representable terms, added in f32 in some
    order (MFMA blocks, then the two slices); any order of T - 1 roundings of relative size u = 2^-24 gives
        |dW - P| <= ((1 + u)^(T-1) - 1) * sum_t |dY[t][n] X[t][k]| <= T u (|dY|^T |X|)[n][k]      for T (T - 1) u <= 1,
    which T = 1088 satisfies (P: the fp64 product; fp64's own error is 2^-29 of this bound).  Two calls give the same bits."""
    yb, xb, P, A = normals
    T = TMAX
    assert T * (T - 1) <= 2 ** 24
    for N, K in ((72, 576), (64, 576), (40, 264)):
        for t in (32, 64, 0, 128):
            assert yv.wgrad_route(T, N, K, t).slices == 2
            got, _ = _launch(yv, yb, xb, T, N, K, t)
            err, bound = (got.double() - P[:N, :K]).abs(), T * 2.0 ** -24 * A[:N, :K]
            print(f"N {N} K {K} tile {t}: max err / bound {float((err / bound).max()):.4f}")
            assert bool((err <= bound).all()), (N, K, t, float((err / bound).max()))
            again, _ = _launch(yv, yb, xb, T, N, K, t)
            assert torch.equal(got, again)


def _trainer_pair(yv, opts):
    """One step of two trainers from the same state on the same batch, narrow_wgrad on / off; the arguments of every
    _wgrad_block call of the default one are recorded."""
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    scale, nc, S, B, G = "n", 5, 64, 2, 2
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(DEV)
    ctr = torch.rand(B, G, 2, generator=g) * (S - 30) + 15
    wh = torch.rand(B, G, 2, generator=g) * 20 + 8
    gtb = torch.cat([ctr - wh / 2, ctr + wh / 2], -1).to(DEV)
    gtl = torch.randint(0, nc, (B, G), generator=g, dtype=torch.int32).to(DEV)
    gtn = torch.full((B,), G, dtype=torch.int32, device=DEV)
    out = []
    with options(yv, **opts):
        for narrow in (True, False):
            tr = YoloTrainer(init_yolo_train_state(scale, nc, seed=3), scale=scale, nc=nc, size=S, batch=B, narrow_wgrad=narrow)
            assert tr.narrow_wgrad is narrow
            calls, inner = [], tr._wgrad_block
            tr._wgrad_block = lambda b, x_buf, x_off, calls=calls, inner=inner: (calls.append((b, x_buf, x_off)), inner(b, x_buf, x_off))
            loss = tr.step(img, gtb, gtl, gtn).cpu().clone()
            torch.cuda.synchronize()
            out.append((tr, loss, tr.grads(), calls))
    return out


def _block_shape(tr, b):
    """(T, N, K) of a block's weight-gradient launch."""
    hin, hout = tr.geom[b.key]
    T = tr.B * (hin + 2) ** 2 if b.k == 3 and b.s == 1 and tr.implicit_wgrad else tr.B * hout * hout
    return (T + 63) // 64 * 64, b.cout, b.taps * b.cin


def test_trainer_narrow_wgrad_bit_equal_at_one_slice(yv):
    """YoloTrainer(narrow_wgrad=True) against the default trainer with every weight gradient in one slice: the same loss and the
    same gradients, bit for bit - and blocks that really leave the 128 x 128 kernel, on all three paths of _wgrad_block."""
    from yvhip.yolo_training import yolo_wgrad_shapes
    (tn, ln, gn, cn), (td, ld, gd, cd) = _trainer_pair(yv, {"wgrad_split_cap": 1, "wgrad_split": 1})
    assert len(cn) == len(cd) == len(tn.blocks)
    with options(yv, wgrad_split_cap=1, wgrad_split=1):
        routes = {b.key: (b, yv.wgrad_route(*_block_shape(tn, b), 0)) for b in tn.blocks}
    assert all(r.slices == 1 for _, r in routes.values())
    narrow = [b for b, r in routes.values() if r.tile_n != 128]
    assert {(b.k, b.s) for b in narrow} >= {(1, 1), (3, 1), (3, 2)}, sorted((b.key, b.k, b.s) for b in narrow)
    assert sorted((T, N, K) for _, T, N, K, _ in yolo_wgrad_shapes("n", 5, 64, 2)) == sorted(_block_shape(tn, b) for b in tn.blocks)
    assert torch.equal(ln, ld) and bool(torch.isfinite(ln).all())
    assert gn.keys() == gd.keys()
    for k in gn:
        assert torch.equal(gn[k], gd[k]), k


def test_trainer_narrow_wgrad_default_slices(yv):
    """The same pair under the default slice rule: the two trainers run the same forward and data-gradient kernels, so every
    weight-gradient launch has the same operands in both, and each result is within T u |dz|^T |x| of the exact product
    (test_narrow_tiles_within_the_f32_summation_bound; T (T - 1) u <= 1 for these shapes).  Hence, per convolution,
        ||dW_narrow - dW_default|| <= 2 T u || |dz|^T |x| ||,    u = 2^-24, T the rows the launch walks,
    which the rel-L2 distance (times ||dW_default||, so that an all-zero gradient needs no special case) is held to, |dz|^T |x|
    computed in fp64 from the operands the default trainer's launch read."""
    (tn, ln, gn, _), (td, ld, gd, calls) = _trainer_pair(yv, {})
    assert torch.equal(ln, ld)                                  # the loss does not depend on the weight gradients
    checked = nonzero = 0
    for b, x_buf, x_off in calls:
        T, N, K = _block_shape(td, b)
        assert T * (T - 1) <= 2 ** 24
        hin, hout = td.geom[b.key]
        Tp = (td.B * hout * hout + 63) // 64 * 64
        if b.k == 1:
            x = x_buf[:Tp, x_off:x_off + b.cin]
        else:
            x = torch.zeros(Tp, 9 * b.cin, dtype=torch.bfloat16, device=DEV)
            yv.im2col3(yv.mview(x_buf, x_off, b.cin), td.B, hin, hin, b.s, x)
        A = td.dz[b.key][:Tp].double().abs().t() @ x.double().abs()
        name = b.key + (".conv.weight" if b.bn else ".weight")
        A = A.view(b.cout, b.k, b.k, b.cin)[:b.cout_real, :, :, :b.cin_real].permute(0, 3, 1, 2).cpu()     # the layout of grads()
        wn, wd = gn[name].double(), gd[name].double()
        assert wn.shape == A.shape
        # rel-L2 times ||dW_default||: a scale without an assigned target has an all-zero box-branch gradient in both trainers
        dist, bound = float((wn - wd).norm()), 2 * T * 2.0 ** -24 * float(A.norm())
        print(f"{name}: ||dW_narrow - dW_default|| {dist:.3g} bound {bound:.3g} ||dW_default|| {float(wd.norm()):.3g}")
        assert dist <= bound, (name, dist, bound)
        nonzero += float(wd.norm()) > 0
        checked += 1
    assert checked == len(td.blocks) and nonzero >= checked - 6
    for k in gn:                                               # BatchNorm and bias gradients do not come from wgrad
        if not (k.endswith("conv.weight") or (k.endswith(".weight") and ".bn." not in k)):
            assert torch.equal(gn[k], gd[k]), k
