"""Cases of the mid-M MXFP8 route step ("linear_mx_mid", gemm_mx_mid_kernel), shared by
test_mx_mid_routes_cpu.py and test_gpu_mx_mid.py.  Operands, references and planted scale faults are mx_exact's own (its
docstring states the construction); this module adds the shapes and the two faults a K split inside a workgroup can have."""
import torch

import mx_exact as mx

MID_SHAPES = {                       # M, N, K
    "m197": (197, 192, 128),         # one K step (group 1 adds zeros); below 256 rows; three column tiles; N % 128 != 0
    "m300": (300, 384, 384),         # three steps (group 1 idles through the last trip); last row tile 44 rows; N % 128 == 0 (_q)
    "m449": (449, 128, 640),         # five steps; last row tile one row
    "m130": (130, 256, 1024),        # eight steps
}
M_DEV = {"m197": (3, 50), "m300": (3, 77), "m449": (3, 130), "m130": (3, 29)}       # (count, m_mul): the cut inside a 64-row tile
Q_SHAPES = ("m300", "m130")          # N % 128 == 0: yv_linear_mxfp8_q
OPTIONS_ON = dict(linear_mx_mid=4096, linear_mx_mid_fill=1 << 20)

# the classifier's block products (N, K) per embedding width, at the engine's flags (bias added by the wrappers)
MODELS = {"vit_base_patch16_224": (768, 197), "vit_base_patch8_224": (768, 785), "vit_large_patch16_224": (1024, 197)}
CROPS = tuple(range(1, 33))


def products(yv, D):
    """(name, N, K, flags, _q form) of the four block products of an mxfp8 engine of width D."""
    B = yv.EPI_BIAS
    return [("qkv", 3 * D, D, B, False), ("proj", D, D, B | yv.EPI_RES_F32, False), ("fc1", 4 * D, D, B | yv.EPI_GELU, True),
            ("fc2", D, 4 * D, B | yv.EPI_RES_F32, False)]


def lin_data(shape: str):
    """mx_exact.lin_data (its builder, its preconditions, its cache) for a shape of MID_SHAPES."""
    mx.LIN_SHAPES[shape] = MID_SHAPES[shape]
    try:
        return mx.lin_data(shape)
    finally:
        del mx.LIN_SHAPES[shape]


def emulate_split(d, fault=None):
    """a w^T + bias from the quantised bytes and scales as the kernel sums them: the 128-element K steps dealt to two groups.
    fault "lost_group": the odd K steps are dropped; "wrong_exchange": rows 0 .. 15 and 16 .. 31 of every 32-row wave tile swap."""
    from mx_reference import dequant, emulate_quant_rows
    ad = dequant(*emulate_quant_rows(d["a"])).float()
    wd = dequant(*emulate_quant_rows(d["w"])).float()
    out = torch.zeros(d["M"], d["N"])
    for h in (0, 1):
        for kt in range(h, d["K"] // 128, 2):
            if fault == "lost_group" and h == 1:
                continue
            out += ad[:, kt * 128:(kt + 1) * 128] @ wd[:, kt * 128:(kt + 1) * 128].t()
    out += d["bias"]
    if fault == "wrong_exchange":
        M = d["M"]
        src = torch.arange(M) ^ 16
        src = torch.where(src < M, src, torch.arange(M))             # (the partner row of a ragged last tile may not exist)
        out = out[src]
    return out
