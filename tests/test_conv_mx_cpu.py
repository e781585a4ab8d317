"""CPU-side checks of the MXFP8 detector: the layer plan of YoloEngine(dtype="mxfp8"), the weight packing of the MX
convolution and its C ABI (no compute calls without a GPU)."""
import ctypes

import torch

import yvhip
from yvhip import engines


def _c2f(idx, n, fused=False):
    if fused:
        return []
    keys = [f"model.{idx}.cv1.conv"]
    for j in range(n):
        keys += [f"model.{idx}.m.{j}.cv1.conv", f"model.{idx}.m.{j}.cv2.conv"]
    return keys + [f"model.{idx}.cv2.conv"]


def _head():
    return [k for s in range(3) for k in (f"det{s}.0", f"model.22.cv2.{s}.1.conv", f"model.22.cv3.{s}.1.conv")]


def test_mx_conv_plan_eligible_n():
    # stem (16 channels out) -> model.1 stays bf16; model.2 / model.4 are fused C2f blocks (one launch each)
    exp = (["model.3.conv", "model.5.conv"] + _c2f(6, 2) + ["model.7.conv"] + _c2f(8, 1) + ["model.9.cv1.conv"]
           + _c2f(12, 1) + _c2f(15, 1) + ["model.16.conv"] + _c2f(18, 1) + ["model.19.conv"] + _c2f(21, 1) + _head())
    assert engines.mx_conv_plan("n", 5, speed_filter=False, min_width=0) == exp


def test_mx_conv_plan_eligible_s():
    # stem writes 32 channels: model.1 is eligible; model.2 (c = 32, n = 1) is a fused block
    exp = (["model.1.conv", "model.3.conv"] + _c2f(4, 2) + ["model.5.conv"] + _c2f(6, 2) + ["model.7.conv"] + _c2f(8, 1)
           + ["model.9.cv1.conv"] + _c2f(12, 1) + _c2f(15, 1) + ["model.16.conv"] + _c2f(18, 1) + ["model.19.conv"]
           + _c2f(21, 1) + _head())
    assert engines.mx_conv_plan("s", 5, speed_filter=False, min_width=0) == exp


def test_mx_conv_plan_eligible_m():
    # stem 48 channels -> model.1 bf16; model.2 has c = 48 (chunks straddle the 32-channel scale blocks): all bf16
    plan = engines.mx_conv_plan("m", 5, speed_filter=False, min_width=0)
    exp = (["model.3.conv"] + _c2f(4, 4) + ["model.5.conv"] + _c2f(6, 4) + ["model.7.conv"] + _c2f(8, 2)
           + ["model.9.cv1.conv"] + _c2f(12, 2) + _c2f(15, 2) + ["model.16.conv"] + _c2f(18, 2) + ["model.19.conv"]
           + _c2f(21, 2) + _head())
    assert plan == exp
    assert not any(k.startswith(("model.0.", "model.1.", "model.2.")) for k in plan)
    assert "model.9.cv2.conv" not in plan                                  # SPPF's pooled chunks stay bf16
    assert not any(k.endswith((".2", ".2.pad")) and k.startswith("model.22.") for k in plan)   # the detect tail's 1 x 1s


def _bottlenecks(idx, n):
    return [f"model.{idx}.m.{j}.cv{k}.conv" for j in range(n) for k in (1, 2)]


def test_mx_conv_plan_shipped():
    """The shipped plans: no 1 x 1 layer (measured slower in MX) and no layer narrower than 96 channels (accuracy)."""
    assert engines.MX_SLOW_KINDS == ((1, 1, False), (1, 1, True)) and engines.MX_MIN_WIDTH == 96
    assert engines.mx_conv_plan("n", 5) == (["model.7.conv"] + _bottlenecks(8, 1) + ["model.19.conv"] + _bottlenecks(21, 1)
                                            + ["det1.0", "det2.0"])
    head3 = [k for s in range(3) for k in (f"det{s}.0", f"model.22.cv3.{s}.1.conv")]
    assert engines.mx_conv_plan("s", 5) == (["model.5.conv"] + _bottlenecks(6, 2) + ["model.7.conv"] + _bottlenecks(8, 1)
                                            + _bottlenecks(12, 1) + ["model.16.conv"] + _bottlenecks(18, 1) + ["model.19.conv"]
                                            + _bottlenecks(21, 1) + head3)
    assert engines.mx_conv_plan("m", 5) == (["model.3.conv"] + _bottlenecks(4, 4) + ["model.5.conv"] + _bottlenecks(6, 4)
                                            + ["model.7.conv"] + _bottlenecks(8, 2) + _bottlenecks(12, 2) + _bottlenecks(15, 2)
                                            + ["model.16.conv"] + _bottlenecks(18, 2) + ["model.19.conv"] + _bottlenecks(21, 2)
                                            + head3)
    for scale in "nsm":
        assert not any(k.endswith(("cv1.conv", "cv2.conv")) and ".m." not in k for k in engines.mx_conv_plan(scale, 5))


def test_mx_conv_plan_reads_only_32_aligned_views():
    """Every MX convolution of every scale reads channel counts / offsets that are multiples of 32 (the engine's own
    launch list, without a device)."""
    for scale in "nsm":
        plan = set(engines.mx_conv_plan(scale, 5, speed_filter=False, min_width=0))
        convs = {e.key: e for e in engines.detect_launches(scale, 5) if isinstance(e, engines.Conv)}
        assert plan <= set(convs)
        for key in plan:
            for _, off, c, _ in convs[key].srcs:
                assert off % 32 == 0 and c % 32 == 0, (scale, key)


def test_conv_weight_padding():
    w = torch.randn(96, 9 * 96).to(torch.bfloat16)                       # K = 864 -> 896
    p = yvhip.pad_k128(w)
    assert p.shape == (96, 896) and torch.equal(p[:, :864], w) and (p[:, 864:] == 0).all()
    w1 = torch.randn(64, 256).to(torch.bfloat16)
    assert yvhip.pad_k128(w1) is w1                                        # already whole K steps


def test_conv_mx_abi_symbols():
    lib = ctypes.CDLL(yvhip.LIB_PATH)
    for name in ("yv_quant_mxfp8_map", "yv_conv2d_mxfp8", "yv_conv2d_mxfp8_instance"):
        assert hasattr(lib, name) and name in yvhip._SIGS and name in yvhip.header_symbols()
    assert [f for f, _ in yvhip.yv_mx_view._fields_] == ["q", "s", "ld", "c", "up"]
    assert len(yvhip._SIGS["yv_conv2d_mxfp8"][1]) == 21


def test_conv_mx_argument_validation_without_gpu():
    assert yvhip.lib.yv_conv2d_mxfp8(None, None, 1, 8, 8, 3, 1, None, None, 128, None, 64, None, 64, None, None, 0, None, 0,
                                     0, None) == -1
    assert yvhip.lib.yv_quant_mxfp8_map(None, 64, 10, 64, None, 64, None, None) == -1
    assert yvhip.lib.yv_conv2d_mxfp8_instance(64, 80, 80, 3, 1, 48, 48) == -1             # Cin not a multiple of 32
    assert yvhip.lib.yv_conv2d_mxfp8_instance(64, 80, 80, 3, 1, 96, 96) == 1              # large map, Cout > 64
    assert yvhip.lib.yv_conv2d_mxfp8_instance(64, 20, 20, 3, 1, 288, 288) == 0
