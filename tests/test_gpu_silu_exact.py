"""yv_c2f_fused, the same block layer by layer (yv_conv2d x (2 + 2n)) and the matrix-pipe stem against the float64 references
of silu_exact.py, element for element: every pre-activation is >= 24, where the kernels' SiLU returns its argument bit for bit,
and every sum is exact in f32 whatever its order (see silu_exact.py; test_silu_exact_cpu.py shows the gate can fail).  Every
comparison is torch.equal; every output buffer is prefilled with 0.5, which no result equals, and carries a spare image (and, in
the strided cases, spare channels) that must keep it.

test_premise_* run first: the identity of SiLU on the device is what everything else here rests on."""
import ctypes as C

import pytest
import torch

import silu_exact as se

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = se.SENTINEL
SHIPPED = {"conv_dma": 8, "conv_splitk": 0, "staged_epilogue": 1}
COMPARED = {}


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    yield yvhip
    print("\nelements compared, per kernel instance:")
    for k in sorted(COMPARED):
        print(f"  {k}: {COMPARED[k]}")
    print(f"  total: {sum(COMPARED.values())}")


class Options:
    """Shipped options overridden by kw; previous values restored on exit (as test_gpu_conv_routes.py)."""

    def __init__(self, yv, **kw):
        self.yv, self.want = yv, dict(SHIPPED, **kw)

    def __enter__(self):
        self.old = {k: self.yv.get_option(k) for k in self.want}
        try:
            for k, v in self.want.items():
                self.yv.set_option(k, v)
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.yv.set_option(k, v)
        return False


def bf(t):
    return t.to(torch.bfloat16)


def tally(key, n):
    COMPARED[key] = COMPARED.get(key, 0) + n


def premise_values():
    """24, 25, .., 256 and the powers of two up to 4096 (all bf16 values), padded with 24 to a multiple of 64."""
    v = [float(i) for i in range(24, 257)] + [512.0, 1024.0, 2048.0, 4096.0]
    v += [24.0] * (-len(v) % 64)
    t = torch.tensor(v)
    assert torch.equal(bf(t).float(), t)
    return t


def fused(yv, c, n, x, ldx, B, H, W, w1, b1, wm, bm, w2, b2, out, ldo):
    """yv_c2f_fused on channel slices: x / out are tensors whose data_ptr is the slice's first element."""
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    p = lambda t: C.c_void_p(t.data_ptr())
    yv.check(yv.lib.yv_c2f_fused(p(x), ldx, B, H, W, c, n, p(w1), p(b1), arr(wm), arr(bm), p(w2), p(b2), p(out), ldo, yv._st()),
             "yv_c2f_fused")


# ------------------------------------------------------------------------------------------------ premise
def test_premise_silu_is_the_identity_from_24(yv):
    """silu_f of the layer kernels (csrc/gemm.hip): 1 x 1 convolution with the identity as weight and no bias, f32 output."""
    vals = premise_values()
    x = bf(vals.view(1, 1, -1, 32)).to(DEV)
    npix = x.shape[2]
    out = torch.full((1, 1, npix, 32), SENTINEL, dtype=torch.float32, device=DEV)
    with Options(yv):
        yv.conv2d(yv.view(x, 0, 32), None, 1, 1, npix, 1, 1, bf(torch.eye(32)).to(DEV), torch.zeros(32, device=DEV), out, 0,
                  yv.EPI_SILU | yv.EPI_OUT_F32)
    torch.cuda.synchronize()
    got = out.cpu().view(-1)
    bad = (got != vals).nonzero().view(-1).tolist()
    print(f"\nsilu_f: {len(vals) - len(bad)} of {len(vals)} values returned bit for bit")
    assert not bad, [(float(vals[i]), float(got[i])) for i in bad[:16]]


@pytest.mark.parametrize("c,n", se.C2F_INSTANCES)
def test_premise_c2f_silu_is_the_identity_from_24(yv, c, n):
    """c2f_silu (csrc/c2f.hip) at its three sites - cv1, the 3 x 3 layers, cv2 - in a block whose answer is known: cv1 the
    identity, the 3 x 3 weights zero with bias 24 (t = 24, y(j+2) = bf16(24 + y(j+1))), cv2 picking y0 into its first c channels
    and y(n+1) into the others."""
    vals = premise_values()
    C1 = 2 * c
    half = vals.view(1, 1, -1, c)
    W = half.shape[2]
    x = bf(torch.cat([half, half], -1)).to(DEV)
    w1, b1 = bf(torch.eye(C1)).to(DEV), torch.zeros(C1, device=DEV)
    wm = [torch.zeros(c, 9 * c, dtype=torch.bfloat16, device=DEV) for _ in range(2 * n)]
    bm = [torch.full((c,), 24.0, device=DEV) for _ in range(2 * n)]
    w2 = torch.zeros(C1, (2 + n) * c)
    w2[:c, :c] = torch.eye(c)
    w2[c:, (n + 1) * c:] = torch.eye(c)
    out = torch.full((1, 1, W, C1), SENTINEL, dtype=torch.bfloat16, device=DEV)
    yv.c2f_fused(x, c, n, w1, b1, wm, bm, bf(w2).to(DEV), torch.zeros(C1, device=DEV), out)
    torch.cuda.synchronize()
    y = half
    for _ in range(n):
        y = bf(24.0 + y).float()
    want = torch.cat([half, y], -1)
    got = out.float().cpu()
    bad = (got != want).nonzero()
    assert len(bad) == 0, [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:16]]


# ------------------------------------------------------------------------------------------------ fused C2f
def c2f_device(case):
    d = dict(xbuf=bf(case["xbuf"]).to(DEV), w=[bf(w).to(DEV) for w in case["w"]], b=[b.to(DEV) for b in case["b"]])
    assert all(torch.equal(a.float().cpu(), w) for a, w in zip(d["w"], case["w"])) and torch.equal(d["xbuf"].float().cpu(), case["xbuf"])
    return d


def check_c2f_output(case, buf, want, what):
    """buf (B + 1, H, W, out_ld): channels [out_off, out_off + 2c) of the first B images equal `want`; all else is the sentinel."""
    B, C1, off = case["B"], 2 * case["c"], case["out_off"]
    buf = buf.float().cpu()
    got = buf[:B, ..., off:off + C1].double()
    gaps = torch.cat([buf[:B, ..., :off], buf[:B, ..., off + C1:]], -1)
    assert bool((gaps == SENTINEL).all()), (case["name"], what, "wrote outside its channels")
    assert bool((buf[B] == SENTINEL).all()), (case["name"], what, "wrote past the last image")
    assert not bool((got == SENTINEL).any()), (case["name"], what, "left outputs unwritten")
    if not torch.equal(got, want):
        raise AssertionError(what + " " + se.describe_c2f_mismatch(case, got, want))
    return got.numel()


@pytest.mark.parametrize("args", se.c2f_cases(), ids=lambda a: se.c2f_name(*a))
def test_c2f_fused_exact(yv, args):
    case = se.build_c2f(*args)
    c, n, B, H, W = (case[k] for k in ("c", "n", "B", "H", "W"))
    d = c2f_device(case)
    out = torch.full((B + 1, H, W, case["out_ld"]), SENTINEL, dtype=torch.bfloat16, device=DEV)
    x = d["xbuf"][..., case["x_off"]:]
    fused(yv, c, n, x, d["xbuf"].shape[-1], B, H, W, d["w"][0], d["b"][0], d["w"][1:-1], d["b"][1:-1], d["w"][-1], d["b"][-1],
          out[..., case["out_off"]:], case["out_ld"])
    torch.cuda.synchronize()
    tally(f"c2f_fused_kernel<{c}, {n}, 16>", check_c2f_output(case, out, case["ref"], "yv_c2f_fused"))


# ------------------------------------------------------------------------------------------------ layer by layer
def run_layers(yv, case, d):
    """The block as the engine runs it without fusion; returns (out buffer, y buffer [y0 | .. | y(n+1)], shortcut layers staged)."""
    c, n, B, H, W = (case[k] for k in ("c", "n", "B", "H", "W"))
    C1, CY = 2 * c, (2 + n) * c
    y = torch.full((B + 1, H, W, CY), SENTINEL, dtype=torch.bfloat16, device=DEV)
    t = torch.full((B, H, W, c), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B + 1, H, W, case["out_ld"]), SENTINEL, dtype=torch.bfloat16, device=DEV)
    w, b = d["w"], d["b"]
    route = yv.conv2d_instance(B, H, W, 3, 1, c, 0, c, CY, CY, yv.EPI_SILU | yv.EPI_RES_BF16)
    yv.conv2d(yv.view(d["xbuf"], case["x_off"], C1), None, B, H, W, 1, 1, w[0], b[0], y, 0, yv.EPI_SILU)
    for j in range(n):
        src = (1 + j) * c
        yv.conv2d(yv.view(y, src, c), None, B, H, W, 3, 1, w[1 + 2 * j], b[1 + 2 * j], t, 0, yv.EPI_SILU)
        yv.conv2d(yv.view(t, 0, c), None, B, H, W, 3, 1, w[2 + 2 * j], b[2 + 2 * j], y, src + c, yv.EPI_SILU | yv.EPI_RES_BF16,
                  res=y, res_c_off=src)
    yv.conv2d(yv.view(y, 0, CY), None, B, H, W, 1, 1, w[-1], b[-1], out, case["out_off"], yv.EPI_SILU)
    torch.cuda.synchronize()
    return out, y, bool(route & yv.CONV_STAGED)


@pytest.mark.parametrize("args", se.c2f_cases(), ids=lambda a: se.c2f_name(*a))
def test_c2f_layer_by_layer_exact(yv, args):
    """The same cases through yv_conv2d, under the shipped options and with staged_epilogue = 0.  The rounding rule of the shortcut
    is the one the route code of its layer names (test_gpu_conv_routes.py::test_shortcut_rounding_rule): bf16(bf16(pre) + y)
    where the staged epilogue runs, bf16(pre + y) - the rule of c2f.hip - elsewhere; at c = 16 / 32 the shortcut layers run in
    16- / 32-wide tiles, which have no staged epilogue, so both option sets must give the single-rounding reference and the
    layer kernels and the fused kernel meet in one third party.  Without the staged epilogue the answer must be the
    single-rounding one whatever the route."""
    case = se.build_c2f(*args)
    d = c2f_device(case)
    for opts in ({}, dict(staged_epilogue=0)):
        with Options(yv, **opts):
            out, y, staged = run_layers(yv, case, d)
        assert not (staged and opts), (case["name"], "a staged route with staged_epilogue = 0")
        want = case["ref_staged"] if staged else case["ref"]
        what = f"yv_conv2d x {2 + 2 * case['n']} ({opts or 'shipped options'}, shortcut {'staged' if staged else 'direct'})"
        nout = check_c2f_output(case, out, want, what)
        ys = se.c2f_chain(case["x"], case["w"], case["b"], case["c"], case["n"], staged=staged)[1][-1]["inp"]
        assert torch.equal(y[:case["B"]].float().cpu().double(), ys.permute(0, 2, 3, 1)), (case["name"], what, "y0 .. y(n+1)")
        assert bool((y[case["B"]] == SENTINEL).all())
        tally(f"yv_conv2d layers c={case['c']} n={case['n']}", nout + ys.numel())


# ------------------------------------------------------------------------------------------------ matrix-pipe stem
@pytest.mark.parametrize("args", se.stem_cases(), ids=lambda a: se.stem_name(*a))
def test_stem_mfma_exact(yv, args):
    case = se.build_stem(*args)
    B, H, W, cout, ld = (case[k] for k in ("B", "H", "W", "cout", "ld"))
    assert W % 128 == 0                                     # the dispatch rule of yv_stem_conv: else this would be the scalar kernel
    Ho, Wo = H // 2, W // 2
    img = case["img"].to(DEV)
    assert img.data_ptr() % 8 == 0
    out = torch.full((B + 1, Ho, Wo, ld), SENTINEL, dtype=torch.bfloat16, device=DEV)
    yv.stem_conv(img, case["w"].to(DEV), case["b"].to(DEV), out[:B])
    torch.cuda.synchronize()
    buf = out.float().cpu()
    got = buf[:B, ..., :cout].double()
    assert bool((buf[:B, ..., cout:] == SENTINEL).all()) and bool((buf[B] == SENTINEL).all()), case["name"]
    chunks = B * Ho * Wo // 64
    if args[:4] == se.STEM_GRID_STRIDE:                     # the chunks past the grid's 2048 x 4 slots: a wave's second trip
        assert chunks > se.STEM_GRID_SLOTS
        rows = got.view(B * Ho, Wo, cout)[se.STEM_GRID_SLOTS * 64 // Wo:]
        assert rows.shape[0] * Wo // 64 == chunks - se.STEM_GRID_SLOTS
        assert torch.equal(rows, case["ref"].view(B * Ho, Wo, cout)[se.STEM_GRID_SLOTS * 64 // Wo:]), "second trip of the grid-stride loop"
        print(f"\n{case['name']}: {chunks} chunks on {se.STEM_GRID_SLOTS} grid slots")
    if not torch.equal(got, case["ref"]):
        bad = (got != case["ref"]).nonzero()
        b, y, x, ch = bad[0].tolist()
        raise AssertionError(f"{case['name']}: {len(bad)} of {got.numel()} values differ; first: image {b}, row {y}, column {x} (chunk "
                             f"{((b * Ho + y) * Wo + x) // 64}, pixel {x % 64} of it), channel {ch}: got {float(got[b, y, x, ch])}, "
                             f"want {float(case['ref'][b, y, x, ch])}")
    tally(f"stem_mfma_kernel<{cout}>", got.numel())
