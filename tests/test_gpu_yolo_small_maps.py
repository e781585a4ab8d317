"""YoloEngine(small_maps=True): the detector with the small-map convolution tiles (option "conv_small" around its pass) against
oracle/yolo.py - the comparisons and limits of tests/test_gpu_models.py::test_yolo_engine_vs_oracle - plus what makes the flag
safe to carry: launches of the two lowest levels really take the new kernels, the option reads 0 again after a call (also one
that raises), the environment variable switches it, and an engine built without it gives the default engine's bits."""
import pytest
import torch

from oracle import yolo as oy
from rect_reference import decode_hw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12))


def small_map_codes(yv, eng, B):
    """Route code of every bf16 Conv entry of the engine's launch list under its option, by level (the output grid's stride)."""
    from yvhip import engines
    flat = eng._buffers(B)["flat"]
    by_level = {}
    old = yv.get_option("conv_small")
    yv.set_option("conv_small", engines.SMALL_MAP_PIXELS)
    try:
        for e in engines.detect_launches(eng.scale, eng.nc, bool(eng.fused_c2f), not eng.fused_tail):
            if type(e) is not engines.Conv or e.key in eng.wq:
                continue
            c = [s[2] for s in e.srcs]
            ld = flat[e.out].shape[-1]
            code = yv.conv2d_instance(B, eng.hw[0] // e.down, eng.hw[1] // e.down, e.k, e.stride, c[0], c[1] if len(c) > 1 else 0,
                                      e.cout, ld, ld if e.res_off is not None else 0, e.flags)
            by_level.setdefault(e.down, []).append(code & 15)
    finally:
        yv.set_option("conv_small", old)
    return by_level


@pytest.mark.parametrize("scale,nc,size,B", [("n", 5, 128, 2), ("s", 80, 64, 1), ("n", 5, (96, 160), 1)])
def test_small_maps_engine_vs_oracle(scale, nc, size, B):
    import yvhip as yv
    from yvhip import engines
    H, W = (size, size) if isinstance(size, int) else size
    sd = oy.init_state(scale, nc, seed=7)
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    raw, outs = oy.forward_raw(sd, oy.blob(img), scale, nc, return_feats=True)
    eng = engines.YoloEngine(sd, scale, nc, size, small_maps=True)
    assert eng.small_maps and eng.resized(size).small_maps
    # not vacuous: launches of each of the two lowest levels take a new code
    levels = small_map_codes(yv, eng, B)
    for down in (16, 32):
        assert any(k in (yv.CONV_SMALL_64, yv.CONV_SMALL_32) for k in levels[down]), (down, levels[down])
    assert yv.get_option("conv_small") == 0
    box_l, cls_l = eng.forward_raw(img.to(DEV))
    torch.cuda.synchronize()
    assert yv.get_option("conv_small") == 0
    bufs = eng._buffers(B)
    for idx in (0, 1, 2, 4, 6, 9, 12, 15, 18, 21):
        got = bufs["out"][idx].float().permute(0, 3, 1, 2).cpu()
        assert rel_l2(got, outs[idx]) < 2e-2, idx
    a0 = 0
    for s, st in enumerate((8, 16, 32)):
        h, w = H // st, W // st
        part = raw[:, :, a0:a0 + h * w].reshape(B, 64 + nc, h, w)
        assert rel_l2(box_l[s].permute(0, 3, 1, 2).cpu(), part[:, :64]) < 2e-2
        assert rel_l2(cls_l[s][..., :nc].permute(0, 3, 1, 2).cpu(), part[:, 64:]) < 2e-2
        a0 += h * w
    eb, es = oy.decode(raw, nc, size) if isinstance(size, int) else decode_hw(raw, nc, H, W)      # (the oracle's decode is square)
    gb, gs = eng(img.to(DEV))
    assert yv.get_option("conv_small") == 0
    assert rel_l2(gs.cpu(), es) < 2e-2
    assert float((gb.cpu() - eb).abs().max()) < 0.02 * max(H, W)       # pixels; DFL expectation of bf16 logits


def test_option_is_restored_after_a_call_that_raises():
    import yvhip as yv
    from yvhip import engines
    eng = engines.YoloEngine(engines.init_yolo_state("n", 5, seed=3), "n", 5, 64, small_maps=True)
    seen = []
    real = eng._launch_list

    def failing(images, tail=True):
        seen.append(yv.get_option("conv_small"))
        raise RuntimeError("inside the pass")

    eng._launch_list = failing
    with pytest.raises(RuntimeError):
        eng(torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV))
    assert seen == [engines.SMALL_MAP_PIXELS] and yv.get_option("conv_small") == 0
    eng._launch_list = real
    with pytest.raises(yv.YvError):
        eng(torch.zeros(1, 32, 64, 3, dtype=torch.uint8, device=DEV))          # the wrong extent: raised inside the pass
    assert yv.get_option("conv_small") == 0


def test_environment_variable_and_default_bits(monkeypatch):
    import yvhip as yv
    from yvhip import engines
    sd = engines.init_yolo_state("n", 5, seed=5, head_gain=4.0)
    monkeypatch.delenv("YV_YOLO_SMALL_MAPS", raising=False)
    plain = engines.YoloEngine(sd, "n", 5, 128)
    assert not plain.small_maps
    monkeypatch.setenv("YV_YOLO_SMALL_MAPS", "1")
    by_env = engines.YoloEngine(sd, "n", 5, 128)
    off = engines.YoloEngine(sd, "n", 5, 128, small_maps=False)
    assert by_env.small_maps and not off.small_maps
    monkeypatch.delenv("YV_YOLO_SMALL_MAPS")
    img = torch.randint(0, 256, (2, 128, 128, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).to(DEV)
    b0, s0 = plain(img)
    b0, s0 = b0.clone(), s0.clone()
    by_env(img)                                                                # a flagged pass in between changes nothing
    assert yv.get_option("conv_small") == 0
    b1, s1 = off(img)
    assert torch.equal(b0, b1) and torch.equal(s0, s1)
    b2, s2 = plain(img)
    assert torch.equal(b0, b2) and torch.equal(s0, s2)
