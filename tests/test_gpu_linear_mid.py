"""GPU checks of the mid-M linear route (gemm_mid_kernel, option "linear_mid"): exact small-integer operands
at every shape at which its tiling or its K split takes another path, agreement with the 128 x 128 route, random bf16 data against
the fp64 product under the gate of test_gpu_dense.py::test_linear_epilogues, and the residual form on a strided f32 stream."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MID_ROWS = 2048


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture()
def mid(yv):
    """linear_mid on for the test, back to what it was afterwards."""
    old = yv.get_option("linear_mid")
    yv.set_option("linear_mid", MID_ROWS)
    try:
        yield yv
    finally:
        yv.set_option("linear_mid", old)


def bf(t):
    return t.to(torch.bfloat16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def assert_mid(yv, M, N, K, flags, **kw):
    for m_dev in (False, True):
        r = yv.linear_route(M, N, K, flags | yv.EPI_BIAS, m_dev=m_dev, **kw)
        assert (r.kernel, r.tile_rows, r.tile_cols, r.splitk) == (yv.LIN_MID, 64, 64, 1)
        assert r.grid == -(-M // 64) * (N // 64)


# M: 257 the first of the route (one live row in the last tile), 320 whole tiles, 321 ragged, 394 two ViT-B/16 crops.
# N: 128 two column tiles, 192 an odd count, 768 / 2304 / 3072 the ViT-B widths.
# K: 64 one K step (the second half has none), 128 one each, 192 uneven, 768 / 3072 the real depths.
SHAPES = [(M, N, K) for M in (257, 321) for N in (128, 192) for K in (64, 128, 192)] + \
         [(320, 768, 768), (394, 768, 3072), (394, 3072, 768), (394, 2304, 768)]
FLAGS = lambda yv, kind: {"plain": 0, "gelu": yv.EPI_GELU, "res": yv.EPI_RES_F32, "f32": yv.EPI_OUT_F32}[kind]


def _integers(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    x = torch.randint(-64, 65, (M, N), generator=g).float()
    return a, w, bias, x


@pytest.mark.parametrize("kind", ["plain", "gelu", "res", "f32"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mid_linear_exact_integer(mid, M, N, K, kind):
    """Operands in [-2, 2], bias in [-8, 8], residual in [-64, 64]: every f32 sum is exact whatever the K split, so bias -> bf16,
    bias + f32 residual read-modify-write and bias -> f32 must EQUAL the integer reference; GELU stays within the project's 3e-3.
    Each case runs contiguous and with strided A rows / output rows, without and with a device row count (rows in between and rows
    past the count keep their sentinel), and twice (bit-identical)."""
    yv = mid
    a, w, bias, x = _integers(M, N, K, M * 7 + N + K)
    lin = a @ w.t() + bias                                     # exact: |sum| < 2^24
    flags = FLAGS(yv, kind)
    f32 = kind in ("res", "f32")
    wd, bd = bf(w).to(DEV), bias.to(DEV)
    fill = 3.0

    def expect(got, rows):
        if kind == "res":
            assert torch.equal(got[:rows], (x + lin)[:rows])
        elif kind == "f32":
            assert torch.equal(got[:rows], lin[:rows])
        elif kind == "plain":
            assert torch.equal(got[:rows], bf(lin).float()[:rows])
        else:
            assert rel_l2(got[:rows], F.gelu(lin)[:rows]) < 3e-3
        if f32:
            assert torch.equal(got[rows:], x[rows:])
        else:
            assert torch.equal(got[rows:], torch.full((M - rows, N), fill))

    counts = [(None, 1, M), (M // 3, 1, M // 3)]               # (device count, m_mul, live rows): M // 3 ends inside a tile
    if M == 394:
        counts.append((1, 197, 197))                           # one crop of two, the engine's own form
    for sa, so in ((1, 1), (3, 2)):                            # row strides: sa * K for A, so * N for the output
        assert_mid(yv, M, N, K, flags, lda=sa * K, ldo=so * N)
        abuf = torch.full((M * sa, K), 7.0, dtype=torch.bfloat16, device=DEV)
        abuf[::sa] = bf(a).to(DEV)
        ad = abuf[::sa]
        for cnt, mul, rows in counts:
            m_dev = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device=DEV)
            outs = []
            for rep in range(2):
                if f32:
                    obuf = torch.full((M * so, N), -5.0, device=DEV)
                    obuf[::so] = x.to(DEV)
                else:
                    obuf = torch.full((M * so, N), fill, dtype=torch.bfloat16, device=DEV)
                yv.linear(ad, wd, bd, obuf[::so], flags=flags, m_dev=m_dev, m_mul=mul)
                torch.cuda.synchronize()
                outs.append(obuf.cpu().float())
            assert torch.equal(outs[0], outs[1])               # determinism
            expect(outs[0][::so], rows)
            if so > 1:                                         # the rows in between are untouched
                between = outs[0].view(M, so, N)[:, 1:]
                assert torch.equal(between, torch.full_like(between, -5.0 if f32 else fill))


@pytest.mark.parametrize("kind", ["plain", "gelu", "res", "f32"])
def test_mid_route_agrees_with_tiled_route(mid, kind):
    """Same integer data through the 128 x 128 route (linear_mid = 0): bit for bit, the GELU form included (one gelu_f)."""
    yv = mid
    M, N, K = 321, 768, 192
    a, w, bias, x = _integers(M, N, K, 4)
    ad, wd, bd = bf(a).to(DEV), bf(w).to(DEV), bias.to(DEV)
    flags = FLAGS(yv, kind)
    new = lambda: x.clone().to(DEV) if kind in ("res", "f32") else torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    o1, o2 = new(), new()
    assert_mid(yv, M, N, K, flags)
    yv.linear(ad, wd, bd, o1, flags=flags)
    yv.set_option("linear_mid", 0)
    try:
        r = yv.linear_route(M, N, K, flags | yv.EPI_BIAS)
        assert (r.kernel, r.tile_rows, r.tile_cols, r.splitk) == (yv.LIN_DMA, 128, 128, 1)
        yv.linear(ad, wd, bd, o2, flags=flags)
    finally:
        yv.set_option("linear_mid", MID_ROWS)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("M,N,K,kind", [(394, 768, 3072, "res"), (394, 3072, 768, "gelu")])
def test_mid_linear_random_against_fp64(mid, M, N, K, kind):
    """Random bf16 operands against the fp64 product, under the gate test_gpu_dense.py::test_linear_epilogues applies to the same
    forms on the 128 x 128 route (GELU -> bf16: rel-L2 < 4e-3; f32 residual: atol 1e-3, rtol 1e-4), and a max error of at most
    twice that route's on the same data: the K split in two changes the f32 rounding of a sum, not its scale."""
    yv = mid
    g = torch.Generator().manual_seed(3)
    a = bf(torch.randn(M, K, generator=g)); w = bf(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g)
    x = torch.randn(M, N, generator=g)
    lin = a.double() @ w.double().t() + bias.double()
    ref = F.gelu(lin) if kind == "gelu" else x.double() + lin
    flags = FLAGS(yv, kind)
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    new = lambda: x.clone().to(DEV) if kind == "res" else torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    o_mid, o_tiled = new(), new()
    assert_mid(yv, M, N, K, flags)
    yv.linear(ad, wd, bd, o_mid, flags=flags)
    yv.set_option("linear_mid", 0)
    try:
        assert yv.linear_route(M, N, K, flags | yv.EPI_BIAS).kernel == yv.LIN_DMA
        yv.linear(ad, wd, bd, o_tiled, flags=flags)
    finally:
        yv.set_option("linear_mid", MID_ROWS)
    torch.cuda.synchronize()
    got, tiled = o_mid.cpu().double(), o_tiled.cpu().double()
    e_mid, e_tiled = float((got - ref).abs().max()), float((tiled - ref).abs().max())
    print(f"{kind} {M}x{N}x{K}: max error mid {e_mid:.3e}, 128 x 128 {e_tiled:.3e}, rel-L2 mid {rel_l2(got, ref):.3e}")
    if kind == "gelu":
        assert rel_l2(got, ref) < 4e-3
    else:
        assert torch.allclose(got, ref, atol=1e-3, rtol=1e-4)
    assert e_mid <= 2 * e_tiled


def test_mid_linear_residual_on_a_strided_stream(mid):
    """The form of test_skinny_linear_residual_cls_stride at M = 300: residual read-modify-write on every third row of a
    (300 * 3, 768) f32 stream, A a compact (300, K) operand, a device count of 250; every other row keeps its contents."""
    yv = mid
    R, S, D, K = 300, 3, 768, 3072
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-2, 3, (R, K), generator=g).float()
    w = torch.randint(-2, 3, (D, K), generator=g).float()
    bias = torch.randint(-8, 9, (D,), generator=g).float()
    x = torch.randint(-64, 65, (R * S, D), generator=g).float()
    lin = a @ w.t() + bias
    xd = x.clone().to(DEV)
    cnt = torch.tensor([250], dtype=torch.int32, device=DEV)
    assert_mid(yv, R, D, K, yv.EPI_RES_F32, ldo=S * D)
    yv.linear(bf(a).to(DEV), bf(w).to(DEV), bias.to(DEV), xd[::S], flags=yv.EPI_RES_F32, m_dev=cnt, m_mul=1)
    torch.cuda.synchronize()
    exp = x.clone()
    exp[::S][:250] += lin[:250]
    assert torch.equal(xd.cpu(), exp)
