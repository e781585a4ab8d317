"""The im2col-free weight gradient by gathered source addresses (yv_wgrad_conv3_gather: gemm_tn_gather_kernel and
gemm_tn_narrow_gather_kernel<64 / 32>) on the GPU.  Every comparison is exact, so there is no tolerance.

Integer operands (x in [-2, 2], dz in {-1, 0, 1}): every product and every f32 partial sum is an integer below 2^24 (asserted
from the shape before the launch), so the result must EQUAL float64 autograd whatever the tile and the slices.  Both operands
have loud first / last rows and columns in every image (+1 / -1 in every channel of the buffer, read or not): a tap that reads
the neighbouring row, or the neighbouring image, where the padding's zero belongs changes a sum.
Normal-distributed operands: bit for bit what yv_im2col3 + yv_wgrad(_tiled) compute from the same operands, for every tile_n -
the route, hence the token slices, is the same, and the LDS holds the same values.
Then YoloTrainer(gather_wgrad=True): every parameter gradient equal to the default trainer's, im2col3 never called, and the
trainer's own checks under YV_YOLO_GATHER_WGRAD=1."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77.0
TILES = (None, 128, 64, 32, 0)
# (B, Hin, Win, stride), Cin, N
SHAPES = [
    pytest.param((1, 6, 6, 2), 8, 16, id="one-tile-mostly-tail-chunk-is-tap"),
    pytest.param((2, 24, 20, 2), 24, 40, id="four-tiles-ragged-K-taps-straddle-tile-edge"),
    pytest.param((2, 7, 5, 2), 32, 8, id="odd-grid-bottom-right-padding-narrow-32"),
    pytest.param((3, 16, 16, 2), 136, 136, id="tap-wider-than-a-K-tile-two-ragged-N-tiles"),
    pytest.param((2, 9, 8, 1), 16, 64, id="stride-1"),
]


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


def r64(n):
    return (n + 63) // 64 * 64


def out_grid(Hin, Win, stride):
    return (Hin - 1) // stride + 1, (Win - 1) // stride + 1


def loud(t):
    """(B, H, W, C): first row / column + 1, last row / column - 1, in every channel."""
    t[:, 0] = 1; t[:, :, 0] = 1; t[:, -1] = -1; t[:, :, -1] = -1
    return t


@functools.lru_cache(maxsize=None)
def operands(grid, Cin, N, integer, sliced):
    """Device buffers of a case, computed once and read-only: x (B*Hin*Win, Cin + pad) and dz (r64(T), N + pad) bf16, the
    operands at channel offset `off` in them, the rest loud; and, for integer data, float64 autograd's dW (N, 9*Cin) on the host."""
    B, Hin, Win, stride = grid
    Hout, Wout = out_grid(Hin, Win, stride)
    T = B * Hout * Wout
    g = torch.Generator().manual_seed(sum(grid) * 1000 + Cin * 10 + N + integer)
    off, pad = (8, 24) if sliced else (0, 0)
    if integer:
        x = loud(torch.randint(-2, 3, (B, Hin, Win, Cin), generator=g).double())
        dz = loud(torch.randint(-1, 2, (B, Hout, Wout, N), generator=g).double())
    else:
        x, dz = torch.randn(B, Hin, Win, Cin, generator=g).bfloat16().double(), torch.randn(B, Hout, Wout, N, generator=g).bfloat16().double()
    xb = loud(torch.full((B, Hin, Win, Cin + pad), 3.0, dtype=torch.float64))
    xb[..., off:off + Cin] = x
    dzb = torch.full((r64(T), N + pad), 1.0, dtype=torch.float64)
    dzb[:T] = loud(torch.full((B, Hout, Wout, N + pad), 2.0, dtype=torch.float64)).view(T, N + pad)
    dzb[:T, off:off + N] = dz.view(T, N)
    dzb[T:, off:off + N] = 0                                    # the ZERO tail of the operand (the rest of the buffer stays loud)
    ref = None
    if integer:
        w = torch.zeros(N, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.permute(0, 3, 1, 2), w, None, stride, 1).backward(dz.permute(0, 3, 1, 2))
        ref = w.grad.permute(0, 2, 3, 1).reshape(N, 9 * Cin).contiguous()
    return xb.view(B * Hin * Win, Cin + pad).bfloat16().to(DEV), dzb.bfloat16().to(DEV), off, ref


def gather(yv, grid, Cin, N, xb, dzb, off, tile_n):
    """yv_wgrad_conv3_gather into a window of a sentinel-filled tensor; asserts that nothing outside the window is written."""
    wb = torch.full((N + 8, 9 * Cin + 16), SENT, device=DEV)
    dw = wb[:N, 4:4 + 9 * Cin]
    yv.wgrad_conv3_gather(dzb[:, off:off + N], yv.mview(xb, off, Cin), dw, *grid, tile_n=tile_n)
    out = dw.clone()
    wb[:N, 4:4 + 9 * Cin] = SENT
    assert bool((wb == SENT).all()), (grid, Cin, N, tile_n)
    return out


def im2col_path(yv, grid, Cin, N, xb, dzb, off, tile_n):
    B, Hin, Win, stride = grid
    col = torch.zeros(dzb.shape[0], 9 * Cin, dtype=torch.bfloat16, device=DEV)
    yv.im2col3(yv.mview(xb, off, Cin), B, Hin, Win, stride, col)
    dw = torch.full((N, 9 * Cin), SENT, device=DEV)
    yv.wgrad(dzb[:, off:off + N], col, dw, T=dzb.shape[0], tile_n=tile_n)
    return dw


def routed_slices(yv, grid, Cin, N, tile_n):
    r, _ = yv.wgrad_conv3_gather_route(*grid, Cin, N, 128 if tile_n is None else tile_n)
    return r.slices


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "channel-slices"])
@pytest.mark.parametrize("grid,Cin,N", SHAPES)
def test_exact_integers_equal_autograd(yv, grid, Cin, N, sliced):
    B, Hin, Win, stride = grid
    Hout, Wout = out_grid(Hin, Win, stride)
    assert B * Hout * Wout * 4 < 2 ** 24                        # |x| <= 2, |dz| <= 1 (2 on no operand element): exact f32 sums
    xb, dzb, off, ref = operands(grid, Cin, N, True, sliced)
    for tile_n in TILES:
        assert routed_slices(yv, grid, Cin, N, tile_n) == 1     # no shape of the table reaches the slice rule's 1,024 rows
        got = gather(yv, grid, Cin, N, xb, dzb, off, tile_n)
        assert torch.equal(got.double().cpu(), ref), (grid, Cin, N, tile_n)


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "channel-slices"])
@pytest.mark.parametrize("grid,Cin,N", SHAPES)
def test_normal_data_has_the_bits_of_the_im2col_path(yv, grid, Cin, N, sliced):
    xb, dzb, off, _ = operands(grid, Cin, N, False, sliced)
    for tile_n in TILES:
        got = gather(yv, grid, Cin, N, xb, dzb, off, tile_n)
        want = im2col_path(yv, grid, Cin, N, xb, dzb, off, tile_n)
        assert bool((want != want.round()).any())               # not an exact-integer case
        assert torch.equal(got, want), (grid, Cin, N, tile_n)


def test_more_than_one_slice(yv):
    """The split over tokens and the reduce pass: "wgrad_split" = 3 forces three slices of one 64-token tile each wherever dW has
    more than 16 output tiles (the 128- and the 32-wide tile of this shape; the 64-wide one has 15 and stays whole).  The im2col
    path is under the same option, so the bits still agree, and the integers still equal autograd."""
    grid, Cin, N = (3, 16, 16, 2), 136, 136
    xi, dzi, off, ref = operands(grid, Cin, N, True, False)
    xn, dzn, _, _ = operands(grid, Cin, N, False, False)
    with options(yv, wgrad_split=3):
        assert [routed_slices(yv, grid, Cin, N, t) for t in TILES] == [3, 3, 1, 3, 3]
        for tile_n in TILES:
            assert torch.equal(gather(yv, grid, Cin, N, xi, dzi, off, tile_n).double().cpu(), ref), tile_n
            assert torch.equal(gather(yv, grid, Cin, N, xn, dzn, off, tile_n), im2col_path(yv, grid, Cin, N, xn, dzn, off, tile_n)), tile_n
    assert yv.get_option("wgrad_split") == 0


def test_rejected_arguments_launch_nothing(yv):
    grid, Cin, N = (2, 8, 8, 2), 16, 32
    x = torch.ones(2 * 8 * 8, Cin, dtype=torch.bfloat16, device=DEV)
    dz = torch.ones(64, N, dtype=torch.bfloat16, device=DEV)
    dw = torch.full((N, 9 * Cin), SENT, device=DEV)
    for bad in (dict(stride=3), dict(tile_n=256), dict(tile_n=48)):
        with pytest.raises(yv.YvError):
            kw = dict(dict(stride=2, tile_n=0), **bad)
            yv.wgrad_conv3_gather(dz, yv.mview(x), dw, 2, 8, 8, kw["stride"], tile_n=kw["tile_n"])
    with pytest.raises(yv.YvError):
        yv.wgrad_conv3_gather(dz[:32], yv.mview(x), dw, *grid)                 # fewer than r64(T) rows of dz
    with pytest.raises(yv.YvError):
        yv.wgrad_conv3_gather(dz, yv.mview(x), dw[:, :136], *grid)             # dw is not (N, 9*Cin)
    torch.cuda.synchronize()
    assert bool((dw == SENT).all())
    yv.wgrad_conv3_gather(dz, yv.mview(x), dw, *grid)
    torch.cuda.synchronize()
    assert bool((dw != SENT).all())


def _gradients(yt, sd, img, monkeypatch, **kw):
    """The flat parameter gradient after one forward + backward from the given state, batch and seeded logit gradients."""
    tr = yt.YoloTrainer({k: v.clone() for k, v in sd.items()}, scale="n", nc=5, size=160, batch=2, **kw)
    if kw.get("gather_wgrad"):
        assert tr.gather_wgrad is True and tr.col.numel() == 8
        assert sorted(tr._gather_blocks) == sorted(["model.0", "model.1", "model.3", "model.5", "model.7", "model.16", "model.19"])

        def im2col3(*a, **k):
            raise AssertionError("im2col3 called with gather_wgrad on")
        monkeypatch.setattr(yt, "im2col3", im2col3)
    else:
        assert tr.gather_wgrad is False and not tr._gather_blocks and tr.col.numel() > 8
    outs = tr.forward(img)
    gr = torch.Generator().manual_seed(12)
    R = [(torch.randn(o[0].shape, generator=gr).bfloat16().float().to(DEV), torch.randn(o[1].shape, generator=gr).bfloat16().float().to(DEV))
         for o in outs]
    tr.backward(R)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return tr.G.cpu().clone()


@pytest.mark.parametrize("narrow", [False, True], ids=["tile-128", "narrow-wgrad"])
def test_trainer_gradients_do_not_change_a_bit(yv, monkeypatch, narrow):
    import yvhip.yolo_training as yt
    monkeypatch.delenv("YV_YOLO_GATHER_WGRAD", raising=False)
    sd = yt.init_yolo_train_state("n", 5, seed=1)
    img = torch.randint(0, 256, (2, 160, 160, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).to(DEV)
    off = _gradients(yt, sd, img, monkeypatch, narrow_wgrad=narrow)
    on = _gradients(yt, sd, img, monkeypatch, narrow_wgrad=narrow, gather_wgrad=True)
    assert float(off.abs().max()) > 0
    assert torch.equal(on, off)


def test_trainer_gather_wgrad_passes_the_trainer_checks(yv, monkeypatch):
    """YV_YOLO_GATHER_WGRAD=1: the project's own trainer checks (tests/test_gpu_yolo_train.py, their tolerances) pass, with seven
    gather launches per backward pass (1 + 12 training steps) and im2col3 never called."""
    import yvhip.yolo_training as yt
    from test_gpu_yolo_train import test_trainer_local_consistency, test_training_steps_reduce_the_loss
    monkeypatch.setenv("YV_YOLO_GATHER_WGRAD", "1")
    calls, real = [0], yt.wgrad_conv3_gather

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    def im2col3(*a, **k):
        raise AssertionError("im2col3 called with YV_YOLO_GATHER_WGRAD=1")

    monkeypatch.setattr(yt, "wgrad_conv3_gather", counted)
    monkeypatch.setattr(yt, "im2col3", im2col3)
    test_trainer_local_consistency(yv, "n", 5, 160, 2)
    test_training_steps_reduce_the_loss(yv)
    assert calls[0] == 7 * 13
