"""The statement of yv_attention_fp8 in numpy, f64: the MXFP8 qkv operand - e4m3 bytes (rows, 3 D) and E8M0
scales in the K-step-major device layout (3 D / 128, rows_pad, 4), as yv_linear_mxfp8_q / yv_quant_mxfp8 write them - is decoded
(mx_reference.dequant), attention runs per (crop, head) on the decoded values, and the result is given as f64, as the bf16 output
and as the MXFP8 output image of the proj operand (mx_reference.emulate_quant_rows on the bf16 rounding).
test_attn_fp8_cpu.py checks it against plain f64 attention; test_gpu_attn_fp8.py measures the kernels against it."""
import numpy as np
import torch

import mx_reference as mxr

HD = 64


def decode(q: torch.Tensor, s_dev: torch.Tensor) -> np.ndarray:
    """bytes (rows, C) uint8 + device scales (C / 128, >= rows, 4) uint8 -> (rows, C) f64."""
    rows = q.shape[0]
    return mxr.dequant(q.cpu(), mxr.scale_rows(s_dev.cpu(), rows)).numpy()


def attention_f64(qkv: np.ndarray, R: int, N: int, H: int, scale: float) -> np.ndarray:
    """qkv (R * N, 3 * H * 64) f64 -> softmax(scale * Q K^T) V per (crop, head), (R * N, H * 64) f64."""
    D = H * HD
    x = qkv.reshape(R, N, 3, H, HD)
    out = np.empty((R, N, H, HD), dtype=np.float64)
    for r in range(R):
        for h in range(H):
            q, k, v = x[r, :, 0, h], x[r, :, 1, h], x[r, :, 2, h]
            s = (q @ k.T) * scale
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[r, :, h] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out.reshape(R * N, D)


def to_bf16(x: np.ndarray) -> torch.Tensor:
    """f64 -> bf16, one rounding to nearest even (f64 -> f32 -> bf16 would round twice)."""
    f = torch.from_numpy(np.ascontiguousarray(x)).double()
    lo = f.float()                                                     # candidates: the bf16 neighbours of the f32 rounding
    b = lo.to(torch.bfloat16)
    up = torch.nextafter(b, torch.full_like(b, float("inf")))
    dn = torch.nextafter(b, torch.full_like(b, float("-inf")))
    best = b.clone()
    for cand in (up, dn):
        closer = (cand.double() - f).abs() < (best.double() - f).abs()
        tie = ((cand.double() - f).abs() == (best.double() - f).abs()) & ((cand.view(torch.int16) & 1) == 0) & \
            ((best.view(torch.int16) & 1) == 1)
        best = torch.where(closer | tie, cand, best)
    return best


def attention_fp8(q: torch.Tensor, s_dev: torch.Tensor, R: int, N: int, H: int, scale: float) -> dict:
    """The outputs of yv_attention_fp8 on (q, s_dev): "f64" (R*N, H*64) numpy, "bf16" the bf16 output, "q" / "s" the MXFP8 image of
    that bf16 output (bytes (R*N, H*64), scale bytes (R*N, H*64 / 32))."""
    out = attention_f64(decode(q[:R * N], s_dev), R, N, H, scale)
    b = to_bf16(out)
    oq, os_ = mxr.emulate_quant_rows(b.float())
    return {"f64": out, "bf16": b, "q": oq, "s": os_}
