"""The tests' MXFP8 reference (mx_reference.py, f64 log2 / ceil) against the definition the kernels compile
(yolov8-vit_amd/csrc/mx_quant.h, mx_block_exp: f32 frexp of amax * (1/448)), over EVERY positive finite bf16 value as a block's
amax.  The GPU tests pin yv_quant_mxfp8 to the reference on data; this pins the two statements of the exponent to each other and
to the property they exist for, amax * 2^-e <= 448 < amax * 2^-(e-1), on all 32 639 inputs."""
import numpy as np
import torch

from mx_reference import block_exp, emulate_quant_rows


def all_bf16_amax() -> np.ndarray:
    """Every positive finite bf16 value (subnormals included), as f32."""
    bits = np.arange(1, 0x7f80, dtype=np.uint32) << 16
    return bits.view(np.float32)


def header_rule(amax: np.ndarray) -> np.ndarray:
    """mx_block_exp in numpy f32 arithmetic (frexp: mant in [0.5, 1))."""
    mant, ex = np.frexp(amax * np.float32(1.0 / 448.0))
    assert mant.dtype == np.float32
    e = np.where(mant == np.float32(0.5), ex - 1, ex)
    return np.where(amax > 0, np.clip(e, -127, 127), -127)


def test_reference_exponent_over_every_bf16_amax():
    amax = all_bf16_amax()
    assert amax.size == 32639 and np.isfinite(amax).all() and (amax > 0).all()
    e_ref = block_exp(torch.from_numpy(amax).double()).numpy().astype(np.int64)
    # unclamped f64 exponent: exact, amax / 448 is far inside the f64 range
    raw = np.ceil(np.log2(amax.astype(np.float64) / 448.0))
    raw = np.where(np.exp2(raw - 1) * 448.0 >= amax, raw - 1, raw)
    clamped = (e_ref == -127) | (e_ref == 127)                  # at a bound of the E8M0 range (the 128 values with e = -127 unclamped count)
    assert int(clamped.sum()) == 1120 and not (raw[~clamped] < -127).any() and not (raw[~clamped] > 127).any()
    free = ~clamped
    a, e = amax[free].astype(np.float64), e_ref[free].astype(np.float64)
    assert (a * np.exp2(-e) <= 448.0).all() and (448.0 < a * np.exp2(-(e - 1))).all()
    assert (e_ref[clamped] == np.clip(raw[clamped], -127, 127)).all()
    assert np.array_equal(e_ref, header_rule(amax).astype(np.int64))


def test_reference_bytes_at_the_edges():
    """All-zero block: scale byte 0 and zero bytes; amax = 448 * 2^k: the element is the format maximum 0x7e, scale 127 + k."""
    x = torch.zeros(5, 32)
    for i, k in enumerate((-3, 0, 5)):
        x[1 + i, 7] = -448.0 * 2.0 ** k
    x[4, 3] = 2.0 ** -20
    q, s = emulate_quant_rows(x)
    assert s.flatten().tolist() == [0, 124, 127, 132, 127 - 28]
    assert int(q[0].sum()) == 0 and q[1:4, 7].tolist() == [0xfe] * 3 and int(q[4, 3]) == 0x78       # 256 = 2^8: e4m3 exponent field 15
