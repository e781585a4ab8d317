"""CPU reference of the library's MXFP8 block format (yolov8-vit_amd/csrc/mx_quant.h; DESIGN.md sections 10 / 11), in f64:
a block is 32 consecutive elements of the last axis, its scale byte e + 127 with e = ceil(log2(amax / 448)) clamped to
[-127, 127] (-127 for an all-zero block), its elements RNE_e4m3(x * 2^-e).  test_mx_reference_cpu.py checks it against the
header's f32 frexp rule for every bf16 amax; the GPU tests pin yv_quant_mxfp8 to it and every fused producer to yv_quant_mxfp8."""
import torch


def block_exp(amax: torch.Tensor) -> torch.Tensor:
    """f64 amax (>= 0) -> f64 exponent e."""
    e = torch.where(amax > 0, torch.ceil(torch.log2((amax / 448.0).clamp_min(1e-300))), torch.full_like(amax, -127.0))
    # log2 of an exact power of two is exact in f64; guard the rounding of ceil() anyway
    return torch.where((amax > 0) & (torch.pow(2.0, e - 1) * 448.0 >= amax), e - 1, e).clamp(-127, 127)


def emulate_quant_rows(x: torch.Tensor):
    """x (..., C) bf16-representable -> (bytes (..., C) uint8, scale bytes (..., C/32) uint8)."""
    shp = x.shape
    b = x.reshape(-1, shp[-1] // 32, 32).double()
    e = block_exp(b.abs().amax(-1))
    q = (b * torch.pow(2.0, -e)[..., None]).float().to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(shp), (e + 127).to(torch.uint8).reshape(*shp[:-1], shp[-1] // 32)


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(bytes (..., C), scale bytes (..., C/32)) -> f64 values."""
    return q.view(torch.float8_e4m3fn).double() * torch.pow(2.0, s.double() - 127.0).repeat_interleave(32, -1)


def emulate_quant(x: torch.Tensor):
    """x (rows, K) bf16-representable f32 -> (bytes (rows, K) uint8, scale bytes (rows, K/32) uint8, dequantised f64)."""
    q, s = emulate_quant_rows(x)
    return q, s, dequant(q, s)


def scale_rows(s: torch.Tensor, rows: int) -> torch.Tensor:
    """Device scale layout (K/128, rows_pad, 4) -> (rows, K/32)."""
    return s[:, :rows].permute(1, 0, 2).reshape(rows, s.shape[0] * 4)


# The blocks at which the exponent rule's two branches decide the byte: all zero (e = -127), amax = +-448 * 2^k (amax / 448 a power
# of two: the mant == 0.5 branch), amax a power of two far below one, and amax 8 among smaller values.
EDGE_KINDS = 7


def edge_rows(rows: int, C: int, seed: int, exact: bool = False) -> torch.Tensor:
    """(rows, C) bf16-representable f32 of log-normal rows whose first and (given room) last EDGE_KINDS blocks, in row-major block
    order, are the edge blocks.  exact: the values are replaced by their dequantised MXFP8 image, i.e. they
    are exact in e4m3 at their block's scale as well, and the edge blocks keep their amax."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 2)).to(torch.bfloat16).float()
    nb = rows * C // 32
    assert nb >= EDGE_KINDS
    b = x.view(nb, 32)
    ramp = torch.linspace(-7, 8, 32).to(torch.bfloat16).float()   # amax 8 = 2^3 at the block's last element, smaller values before
    for base in ([0, nb - EDGE_KINDS] if nb >= 2 * EDGE_KINDS else [0]):
        b[base + 0] = 0
        for i, k in enumerate((-3, 0, 5)):
            b[base + 1 + i] = (b[base + 1 + i] / b[base + 1 + i].abs().max() * 2.0 ** k).to(torch.bfloat16).float()   # |.| <= 2^k
            b[base + 1 + i, (7 * i + 3) % 32] = (448.0 if i != 1 else -448.0) * 2.0 ** k
        b[base + 4, :] = 448.0                                   # every element at the format maximum
        b[base + 5] = 2.0 ** -20 * torch.sign(b[base + 5] + 0.5)
        b[base + 6] = ramp
    if exact:
        x = emulate_quant(x)[2].float() + 0.0                     # (-0 -> +0: a product -0 added to an accumulator's +0 is +0)
        assert torch.equal(x, x.to(torch.bfloat16).float())
    return x


def assert_edge_blocks(x: torch.Tensor):
    """x holds every edge block (the callers' guard against a planted tensor that lost them)."""
    amax = x.reshape(-1, 32).abs().amax(-1)
    for v in (0.0, 56.0, 448.0, 14336.0, 2.0 ** -20, 8.0):
        assert bool((amax == v).any()), v
