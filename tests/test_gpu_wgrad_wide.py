"""The 256 x 128 weight-gradient tiles (gemm_tn_wide_kernel, yv_wgrad_wide, VitTrainer(wide_wgrad=True)) on the GPU.  Small-integer
operands make every sum exact, so those results must EQUAL the fp64 product whatever the tile and the number of token slices; on random operands the wide tile must give the 128 x 128 tile's bits for an equal slice count, and stay inside the
f32 summation bound under its own slice rule."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, KS, TS = (8, 128, 136, 256, 264, 520), (8, 72, 128, 136, 264), (64, 128, 192, 1088)
UNEVEN = (1088, 1032, 648)                               # 5 x 6 = 30 wide tiles, 9 x 6 = 54 tiles of 128 x 128, 17 token tiles
TMAX, NMAX, KMAX, XOFF, WOFF, SENT = 1088, 1032, 648, 8, 8, -77.0


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
    """dY inside a wider buffer (row stride NMAX + 16 > N), X at column XOFF of a wider buffer; integers in [-2, 2] or N(0, 1)."""
    g = torch.Generator().manual_seed(11)
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
    ref = {T: yb[:T, :NS[-1]].double().t() @ xb[:T, XOFF:XOFF + KS[-1]].double() for T in TS}
    ref["uneven"] = yb[:, :NMAX].double().t() @ xb[:, XOFF:XOFF + KMAX].double()
    return yb, xb, ref


@pytest.fixture(scope="module")
def normals():
    yb, xb = _operands("normal")
    y, x = yb[:, :NMAX].double(), xb[:, XOFF:XOFF + KMAX].double()
    return yb, xb, y.t() @ x, y.abs().t() @ x.abs()


def _launch(yv, yb, xb, T, N, K, routed):
    """wgrad_wide (routed: True / False) or wgrad (routed: None) on the slices; returns (dW region, the wider sentinel-filled
    tensor it lives in)."""
    wb = torch.full((N + 8, K + 24), SENT, device=DEV)
    dw = wb[:N, WOFF:WOFF + K]
    if routed is None:
        yv.wgrad(yb[:T, :N], xb[:T, XOFF:XOFF + K], dw)
    else:
        yv.wgrad_wide(yb[:T, :N], xb[:T, XOFF:XOFF + K], dw, routed=routed)
    return dw, wb


def _untouched(wb, N, K):
    c = wb.clone()
    c[:N, WOFF:WOFF + K] = SENT
    return bool((c == SENT).all())


@pytest.mark.parametrize("routed", [False, True])
@pytest.mark.parametrize("T", TS)
def test_wgrad_wide_exact(yv, ints, T, routed):
    """Exact sums: dW must equal the fp64 product for every (N, K) - one to three n tiles and k tiles, every count of live
    fragments that N, K = 8, 72, 128, 136, 264, 520 leave in the last tile - with no slice (T = 64: two stages, nothing in flight
    behind them; 128; 192) and with the slices of the default rule (T = 1088: eight, of two and three token tiles), and nothing
    outside [N, K] is written.  Routed, these shapes (at most 15 tiles of 128 x 128) are yv_wgrad's launch."""
    yb, xb, ref = ints
    split = set()
    for N in NS:
        for K in KS:
            r = yv.wgrad_wide_route(T, N, K, routed=routed)
            if routed:
                assert r == yv.wgrad_route(T, N, K, 128) and r.tile_n == 128
            else:
                assert r.tile_n == 256 and r.tile_k == 128 and r.tiles == -(-N // 256) * -(-K // 128)
                assert r.slices == (8 if T == 1088 else 1), (T, N, K, r)
            split.add(r.slices > 1)
            dw, wb = _launch(yv, yb, xb, T, N, K, routed)
            assert torch.equal(dw.double(), ref[T][:N, :K]), (T, N, K, routed)
            assert _untouched(wb, N, K), (T, N, K, routed)
    assert split == ({True} if T == 1088 else {False})       # over the T cases: the split path and the no-split path are both reached
    if not routed and T == 192:                              # exactly two slices, of one and two token tiles
        with options(yv, wgrad_split=2):
            for N, K in ((520, 264), (136, 72)):
                assert yv.wgrad_wide_route(T, N, K).slices == 2
                dw, wb = _launch(yv, yb, xb, T, N, K, False)
                assert torch.equal(dw.double(), ref[T][:N, :K]) and _untouched(wb, N, K)
    assert yv.get_option("wgrad_split") == 0


@pytest.mark.parametrize("split", [0, 3])
def test_wgrad_wide_uneven_slices(yv, ints, split):
    """17 token tiles over a slice count that does not divide them (the default rule's eight; three forced), 30 wide tiles with a
    partial last n tile (8 live columns) and a partial last k tile (8 live columns).  Routed, a product this
    small is yv_wgrad's launch (54 tiles of 128 x 128 over 17 token tiles), exact as well."""
    yb, xb, ref = ints
    T, N, K = UNEVEN
    with options(yv, wgrad_split=split):
        r = yv.wgrad_wide_route(T, N, K)
        assert r.tile_n == 256 and r.tiles == 30 and r.slices >= 3 and (T // 64) % r.slices != 0, r
        assert r.slices == (3 if split else 8)
        dw, wb = _launch(yv, yb, xb, T, N, K, False)
        assert torch.equal(dw.double(), ref["uneven"]), split
        assert _untouched(wb, N, K)
    with options(yv, wgrad_split=split):
        assert yv.wgrad_wide_route(T, N, K, routed=True) == yv.wgrad_route(T, N, K, 128)
        dw, wb = _launch(yv, yb, xb, T, N, K, True)
        assert torch.equal(dw.double(), ref["uneven"]) and _untouched(wb, N, K)
    assert yv.get_option("wgrad_split") == 0


def test_wide_tiles_give_the_bits_of_the_128_tile(yv, normals):
    """N(0, 1) operands, an equal slice count: the wide kernel runs the 128 x 128 kernel's chain of MFMAs on the same values for
    every dW element (and the slices meet at the same token tiles), so the results are bit-identical."""
    yb, xb, _, _ = normals
    for opts, shapes in (({"wgrad_split_cap": 1, "wgrad_split": 1}, ((TMAX, 520, 264), (TMAX, 256, 128))), ({"wgrad_split": 3}, (UNEVEN,))):
        with options(yv, **opts):
            for T, N, K in shapes:
                want = opts["wgrad_split"]
                assert yv.wgrad_wide_route(T, N, K).slices == want and yv.wgrad_route(T, N, K, 128).slices == want
                assert yv.wgrad_wide_route(T, N, K).tile_n == 256
                base, _ = _launch(yv, yb, xb, T, N, K, None)
                assert float(base.abs().max()) > 1 and bool((base != base.round()).any())      # not an exact-integer case
                got, wb = _launch(yv, yb, xb, T, N, K, False)
                assert torch.equal(got, base), (T, N, K)
                assert _untouched(wb, N, K)
    assert yv.get_option("wgrad_split_cap") == 128 and yv.get_option("wgrad_split") == 0


def test_wide_tiles_within_the_f32_summation_bound(yv, normals):
    """The wide tile's own slice rule (eight slices at T = 1088), N(0, 1) operands.  A product of two bf16 values has at most 16
    significant bits: exact in f32.  dW[n][k] is therefore a sum of T exactly representable terms, added in f32 in some order
    (MFMA blocks, then the slices); any order of T - 1 roundings of relative size u = 2^-24 gives
        |dW - P| <= ((1 + u)^(T-1) - 1) * sum_t |dY[t][n] X[t][k]| <= T u (|dY|^T |X|)[n][k]      for T (T - 1) u <= 1,
    which T = 1088 satisfies (P: the fp64 product; fp64's own error is 2^-29 of this bound).  Two calls give the same bits."""
    yb, xb, P, A = normals
    T = TMAX
    assert T * (T - 1) <= 2 ** 24
    for N, K, routed in ((520, 264, False), (256, 128, False), (1032, 648, False)):
        r = yv.wgrad_wide_route(T, N, K, routed=routed)
        assert r.tile_n == 256 and r.slices == 8
        got, _ = _launch(yv, yb, xb, T, N, K, routed)
        err, bound = (got.double() - P[:N, :K]).abs(), T * 2.0 ** -24 * A[:N, :K]
        print(f"N {N} K {K} routed {routed}: max err / bound {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (N, K, routed, float((err / bound).max()))
        again, _ = _launch(yv, yb, xb, T, N, K, routed)
        assert torch.equal(got, again)


# ------------------------------------------------------------------------------------------------ trainer
NAME, R = "vit_tiny_test", 3                              # patch 16, width 128, depth 2: dW 384 x 128, 128 x 128, 512 x 128, 128 x 512
T_FULL = 640                                              # 3 x 197 tokens, padded to 64


def _problem():
    from yvhip import engines
    sd = engines.init_vit_wrapper_state(NAME, 5, 21)
    g = torch.Generator().manual_seed(R)
    pm = (torch.rand(R * 196, 768, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(DEV)
    return sd, pm, labels


def _train(yv, monkeypatch, **kw):
    """One forward + backward of a fresh trainer -> (trainer, loss, gradients, launches).  Every bf16 weight-gradient launch is
    recorded as (weight name, entry, T, N, K, ||  |dy|^T |x|  || in fp64 from the operands the launch read).  wgrad_wide is
    forced onto the wide tile where the route would send a shape of this tiny model back to 128 x 128 tiles: the comparison
    must not be between a kernel and itself."""
    from yvhip import training
    from yvhip.training import VitTrainer
    sd, pm, labels = _problem()
    tr = VitTrainer(sd, NAME, 5, **kw)
    names = {tr.g(k).data_ptr(): k for k in tr.names}
    launches = []

    def recording(entry):
        real = getattr(yv, entry)

        def wrapper(dy, x, dw, T=None, **k):
            t = dy.shape[0] if T is None else T
            a = float((dy[:t].double().abs().t() @ x[:t].double().abs()).norm())
            launches.append((names[dw.data_ptr()], entry, t, dy.shape[1], x.shape[1], a))
            if entry == "wgrad_wide":
                assert k == {"routed": True}
                return real(dy, x, dw, T=T, routed=False)
            assert not k
            return real(dy, x, dw, T=T)
        return wrapper

    for entry in ("wgrad", "wgrad_wide"):
        monkeypatch.setattr(training, entry, recording(entry))
    tr.forward(pm, R)
    loss = tr.backward(pm, labels, R).clone()
    torch.cuda.synchronize()
    return tr, loss, tr.grad_dict(), launches


def test_trainer_wide_wgrad_bit_equal_at_one_slice(yv, monkeypatch):
    """VitTrainer(wide_wgrad=True) against the default trainer with every weight gradient in one slice: the same loss and the
    same gradients, bit for bit - with wgrad_wide called for every weight gradient, on the wide tile."""
    with options(yv, wgrad_split_cap=1, wgrad_split=1):
        tw, lw, gw, cw = _train(yv, monkeypatch, wide_wgrad=True)
        td, ld, gd, cd = _train(yv, monkeypatch)
        assert tw.wide_wgrad is True and td.wide_wgrad is False
        assert len(cw) == len(cd) == 2 * 4 + 2 and {c[1] for c in cw} == {"wgrad_wide"} and {c[1] for c in cd} == {"wgrad"}
        assert [c[0] for c in cw] == [c[0] for c in cd] and [c[2:5] for c in cw] == [c[2:5] for c in cd]
        shapes = {c[0].split(".", 3)[-1]: c[2:5] for c in cw}
        assert shapes["attn.qkv.weight"] == (T_FULL, 384, 128) and shapes["mlp.fc1.weight"] == (T_FULL, 512, 128)
        assert shapes["mlp.fc2.weight"] == (T_FULL, 128, 512) and shapes["attn.proj.weight"] == (T_FULL, 128, 128)
        for _, _, T, N, K, _ in cw:                           # the launches the wrapper made: forced, wide, one slice like wgrad's
            r = yv.wgrad_wide_route(T, N, K)
            assert r.tile_n == 256 and r.slices == 1 and yv.wgrad_route(T, N, K, 128).slices == 1
    assert torch.equal(lw, ld) and bool(torch.isfinite(lw).all())
    assert gw.keys() == gd.keys()
    for k in gw:
        assert bool(torch.isfinite(gw[k]).all()), k
        assert torch.equal(gw[k], gd[k]), k
    assert all(float(gd[c[0]].abs().max()) > 0 for c in cd)


def test_trainer_wide_wgrad_default_slices(yv, monkeypatch):
    """The same pair under the default slice rules: the two trainers run the same forward and data-gradient kernels, so every
    weight-gradient launch has the same operands in both, and each result is within T u |dy|^T |x| of the exact product
    (test_wide_tiles_within_the_f32_summation_bound; T (T - 1) u <= 1 for these shapes).  Hence, per weight,
        ||dW_wide - dW_default|| <= 2 T u || |dy|^T |x| ||,    u = 2^-24, T the rows the launch walks.
    Every gradient that no weight-gradient launch writes is equal."""
    tw, lw, gw, cw = _train(yv, monkeypatch, wide_wgrad=True)
    td, ld, gd, cd = _train(yv, monkeypatch)
    assert torch.equal(lw, ld)
    assert any(yv.wgrad_wide_route(c[2], c[3], c[4]).slices != yv.wgrad_route(c[2], c[3], c[4], 128).slices for c in cw)
    for (name, _, T, N, K, a), other in zip(cd, cw):
        assert other[0] == name and abs(other[5] - a) <= 1e-12 * a      # the same operands
        assert T * (T - 1) <= 2 ** 24
        dist, bound = float((gw[name].double() - gd[name].double()).norm()), 2 * T * 2.0 ** -24 * a
        print(f"{name} ({T}, {N}, {K}): ||dW_wide - dW_default|| {dist:.3g} bound {bound:.3g} ||dW_default|| {float(gd[name].norm()):.3g}")
        assert dist <= bound, (name, dist, bound)
    written = {c[0] for c in cd}
    assert len(written) == 10
    for k in gw:
        if k not in written:
            assert torch.equal(gw[k], gd[k]), k


@pytest.mark.parametrize("kw", [dict(cls_tail=True), dict(dtype="mxfp8")], ids=["cls_tail", "mxfp8"])
def test_trainer_wide_wgrad_with_the_other_recipes(yv, monkeypatch, kw):
    """One step of wide_wgrad=True with cls_tail=True (the compact cls-row launches: T = 64) and with dtype="mxfp8" (only the
    head and the patch embedding are bf16 weight gradients): finite losses, and every tensor that no bf16 weight-gradient launch
    writes equals the same trainer with wide_wgrad=False."""
    tw, lw, gw, cw = _train(yv, monkeypatch, wide_wgrad=True, **kw)
    td, ld, gd, cd = _train(yv, monkeypatch, wide_wgrad=False, **kw)
    assert bool(torch.isfinite(lw).all()) and torch.equal(lw, ld)
    assert [c[0] for c in cw] == [c[0] for c in cd] and {c[1] for c in cw} == {"wgrad_wide"} and {c[1] for c in cd} == {"wgrad"}
    if "cls_tail" in kw:
        assert len(cw) == 10 and sorted(c[2] for c in cw).count(64) >= 3          # proj, fc1, fc2 of the last block on the cls rows
    else:
        assert [c[0] for c in cw] == ["model.head.weight", "model.patch_embed.proj.weight"]
    written = {c[0] for c in cd}
    for k in gw:
        assert bool(torch.isfinite(gw[k]).all()), k
        if k not in written:
            assert torch.equal(gw[k], gd[k]), k
    for (name, _, T, N, K, a) in cd:
        assert float((gw[name].double() - gd[name].double()).norm()) <= 2 * T * 2.0 ** -24 * a, name
