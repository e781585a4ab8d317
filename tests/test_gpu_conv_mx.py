"""MXFP8 detector convolutions (BASELINE.json configs[4]: FP8 convolutions; YoloEngine(dtype="mxfp8")).

The map quantiser must reproduce a torch emulation of the rule byte for byte; the block-scaled implicit-GEMM convolution must
equal the fp64 convolution of the DEQUANTISED operands up to fp32 accumulation (products of two e4m3 values are exact in
fp32); its MX-map output must be the bf16 output quantised afterwards, byte for byte."""
import pytest
import torch
import torch.nn.functional as F

from mx_reference import assert_edge_blocks, dequant as dequant_map, edge_rows, emulate_quant_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


def dequant_weight(wq: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """(Cout, Kpad) e4m3 + K-step-major scales (Kpad/128, rows_pad, 4) -> (Cout, Kpad) f64."""
    co, kp = wq.shape
    sc = ws[:, :co, :].permute(1, 0, 2).reshape(co, kp // 32)
    return dequant_map(wq, sc)


def _bf16_input(g, B, H, W, ld):
    return (torch.randn(B, H, W, ld, generator=g) * torch.exp(torch.randn(B, H, W, 1, generator=g))).to(torch.bfloat16)


@pytest.mark.parametrize("shape,c_off,c,ld_q", [((2, 5, 7, 96), 0, 96, 96), ((3, 4, 4, 160), 32, 96, 128),
                                                ((1, 9, 9, 640), 128, 512, 512), ((2, 3, 3, 64), 32, 32, 96)])
def test_quant_mxfp8_map_matches_emulation(yv, shape, c_off, c, ld_q):
    g = torch.Generator().manual_seed(sum(shape) + c_off)
    x = _bf16_input(g, *shape)
    x[0, 0, 0, c_off:c_off + 32] = 0                              # an all-zero block
    x[0, 0, 1, c_off:c_off + 32] = 448.0                          # amax exactly at the format maximum (a power-of-two ratio)
    x[-1, -1, -1, c_off + c - 32:c_off + c] = -(2.0 ** -20)       # amax exactly a power of two
    x[-1, 0, 0, c_off:c_off + 32] = torch.linspace(-7, 8, 32)      # amax 8 = 2^3
    qb, sb = emulate_quant_rows(x[..., c_off:c_off + c].float())
    q = torch.full((*shape[:3], ld_q), 0xAB, dtype=torch.uint8, device=DEV)
    s = torch.full((*shape[:3], ld_q // 32), 0xCD, dtype=torch.uint8, device=DEV)
    o = ld_q - c                                                  # write at a channel offset of the map
    yv.quant_mxfp8_map(x.to(DEV), (q, s), c_off, c, o)
    torch.cuda.synchronize()
    q, s = q.cpu(), s.cpu()
    assert torch.equal(q[..., o:o + c], qb) and torch.equal(s[..., o // 32:(o + c) // 32], sb)
    assert (q[..., :o] == 0xAB).all() and (s[..., :o // 32] == 0xCD).all()      # nothing outside the view


# (B, Hout, ksize, stride, sources [(c, up)], Cout, kind, view channel offset of source 0 / its pixel stride)
CASES = [
    (2, 20, 3, 1, [(96, 0)], 96, "f32", (0, 96)),
    (2, 10, 3, 2, [(128, 0)], 64, "f32", (0, 128)),
    (1, 13, 3, 1, [(192, 0)], 192, "res", (0, 192)),              # ragged M (169 rows)
    (2, 10, 3, 1, [(288, 0)], 64, "f32", (0, 288)),
    (2, 10, 1, 1, [(384, 0)], 192, "bf16", (0, 384)),
    (1, 7, 3, 2, [(576, 0)], 576, "f32", (0, 576)),
    (2, 2, 3, 1, [(128, 0)], 64, "f32", (0, 128)),               # a 2 x 2 image
    (2, 9, 3, 2, [(96, 0)], 96, "res", (32, 160)),               # channel offset and pixel stride > C
    (2, 12, 1, 1, [(384, 0), (192, 0)], 192, "bf16", (0, 384)),
    (2, 12, 1, 1, [(576, 1), (384, 0)], 96, "f32", (0, 576)),    # upsampled first source, block straddling the sources
    (2, 8, 1, 2, [(128, 0)], 64, "bf16", (0, 128)),
    (1, 320, 1, 1, [(96, 0)], 128, "bf16", (0, 96)),             # >= 100 k output pixels, Cout > 64: 128-wide tiles
    (1, 320, 3, 1, [(96, 0)], 96, "f32", (0, 96)),
]


def case_instances(yv):
    return {yv.conv2d_mxfp8_instance(B, H, H, k, s, sum(c for c, _ in src), co) for B, H, k, s, src, co, _, _ in CASES}


def _run_case(yv, case, seed, mx_out=False, bf16_out=True):
    B, H, k, s, src, co, kind, (coff, ld0) = case
    g = torch.Generator().manual_seed(seed)
    Hin = H * s
    maps, views, deq = [], [], []
    for i, (c, up) in enumerate(src):
        ld = ld0 if i == 0 else c
        off = coff if i == 0 else 0
        h = Hin >> up
        x = _bf16_input(g, B, h, h, ld).to(DEV)
        m = yv.mx_map(B, h, h, ld, DEV)
        yv.quant_mxfp8_map(x, m)
        maps.append(m)
        views.append(yv.mx_view(m, off, c, up))
        d = dequant_map(m[0][..., off:off + c].cpu(), m[1][..., off // 32:(off + c) // 32].cpu()).to(DEV)
        if up:
            d = d.repeat_interleave(2, 1).repeat_interleave(2, 2)
        deq.append(d)
    cin = sum(c for c, _ in src)
    w = (torch.randn(co, k * k * cin, generator=g) * (2.0 / (k * k * cin)) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(co, generator=g).to(DEV)
    wq, ws = yv.quant_conv_weight_mxfp8(w.to(DEV))
    wd = dequant_weight(wq.cpu(), ws.cpu())[:, :k * k * cin].to(DEV)
    xd = torch.cat(deq, -1).permute(0, 3, 1, 2)                               # (B, Cin, Hin, Win) f64
    cols = F.unfold(xd, k, padding=k // 2, stride=s)                           # (B, Cin*k*k [cin-major], L)
    wk = wd.view(co, k, k, cin).permute(0, 3, 1, 2).reshape(co, cin * k * k)
    ref = (wk @ cols).view(B, co, H, H).permute(0, 2, 3, 1) + bias.double()   # (B, H, W, Cout)
    # fp32 accumulation error scales with sum |a w| (blocks of different taps / pixels carry very different scales)
    mag = (wk.abs() @ cols.abs()).view(B, co, H, H).permute(0, 2, 3, 1) + bias.double().abs()
    flags = yv.EPI_SILU if kind != "f32" or seed % 2 else 0
    if flags:
        ref = ref * torch.sigmoid(ref)
    res = None
    if kind == "res":
        res = torch.randn(B, H, H, co + 32, generator=g).to(torch.bfloat16).to(DEV)
        flags |= yv.EPI_RES_BF16
    out_mx = yv.mx_map(B, H, H, co + 64, DEV) if mx_out else None
    if kind == "f32":
        out = torch.zeros(B, H, H, co, device=DEV)
        flags |= yv.EPI_OUT_F32
    else:
        out = torch.zeros(B, H, H, co + 16, dtype=torch.bfloat16, device=DEV)
    yv.conv2d_mxfp8(views[0], views[1] if len(views) > 1 else None, B, H, H, k, s, wq, ws, bias, out if bf16_out else None,
                    0 if kind == "f32" else 8, flags, res=res, res_c_off=32 if res is not None else 0,
                    out_mx=out_mx, outq_c_off=32 if mx_out else 0)
    torch.cuda.synchronize()
    return out, ref, res, out_mx, flags, mag


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}_H{c[1]}_k{c[2]}s{c[3]}_{'+'.join(str(x) for x, _ in c[4])}_co{c[5]}_{c[6]}"
                                             for c in CASES])
def test_conv2d_mxfp8_matches_dequantised_conv(yv, case):
    out, ref, res, _, flags, mag = _run_case(yv, case, seed=case[1] * 7 + case[5])
    kind = case[6]
    if kind == "f32":
        got = out.double()
        assert torch.allclose(got, ref, rtol=2e-5, atol=2e-5 * float(mag.max())), float((got - ref).abs().max())
    else:
        got = out[..., 8:8 + case[5]].double()
        exp = ref
        if res is not None:
            exp = ref.to(torch.bfloat16).double() + res[..., 32:32 + case[5]].double()
        err = float((got - exp).norm() / exp.norm())
        assert err < 4e-3, err                                             # bf16 output rounding
        assert (out[..., :8] == 0).all() and (out[..., 8 + case[5]:] == 0).all()


def test_conv2d_mxfp8_instances_cover_the_bench_shapes(yv):
    """Every eligible convolution of YOLOv8m at batch 64 and YOLOv8n at batch 32 (640 x 640) dispatches to a kernel instance
    that the parity test above runs."""
    from oracle import yolo
    from yvhip.engines import LAYER_STRIDE
    covered = case_instances(yv)
    seen = set()
    for scale, B in (("m", 64), ("n", 32)):
        for key, cin, cout, k, s in yolo.conv_shapes(scale, 5):
            if cin % 32 or cout % 32:
                continue
            parts = key.split(".")
            idx = int(parts[1])
            st = (8, 16, 32)[int(parts[3])] if idx == 22 else LAYER_STRIDE[idx]
            H = 640 // st
            inst = yv.conv2d_mxfp8_instance(B, H, H, k, s, cin, cout)
            assert inst in covered, (scale, key, inst, covered)
            seen.add(inst)
    assert seen == {0, 1}, seen


@pytest.mark.parametrize("ci", [2, 7, 8, 9, 11])
def test_conv2d_mxfp8_mx_output_is_quantised_bf16_output(yv, ci):
    case = CASES[ci]
    if case[6] == "f32":
        case = case[:6] + ("bf16",) + case[7:]
    out, _, _, out_mx, flags, _ = _run_case(yv, case, seed=ci, mx_out=True)
    co = case[5]
    q, s = out_mx
    want = yv.mx_map(*q.shape[:3], co, DEV)
    yv.quant_mxfp8_map(out, want, 8, co)
    torch.cuda.synchronize()
    assert torch.equal(q[..., 32:32 + co], want[0]) and torch.equal(s[..., 1:1 + co // 32], want[1])
    assert (q[..., :32] == 0).all() and (q[..., 32 + co:] == 0).all()
    # the bf16 output of that launch (MX epilogue) is the bf16 output of the same launch without the MX map (finish_tile)
    plain, _, _, _, _, _ = _run_case(yv, case, seed=ci)
    assert torch.equal(out, plain)
    # the MX map alone (no bf16 store): the same bytes
    _, _, _, only_mx, _, _ = _run_case(yv, case, seed=ci, mx_out=True, bf16_out=False)
    assert torch.equal(only_mx[0], q) and torch.equal(only_mx[1], s)


@pytest.mark.parametrize("bf16_out", [True, False])
def test_conv2d_mxfp8_mx_output_edge_blocks(yv, bf16_out):
    """1 x 1, stride 1, identity weight, zero bias, no SiLU on the dequantised image of a planted tensor (mx_reference.edge_rows: the
    blocks where the exponent rule's branches decide the byte): every output is one exact product, so the MX-map output is the CPU
    reference of the input, with and without the bf16 store.  Ragged M (169 pixels), three blocks per pixel."""
    B, H, C = 1, 13, 96
    x = edge_rows(B * H * H, C, seed=13, exact=True)
    assert_edge_blocks(x)
    qb, sb = emulate_quant_rows(x)
    m = yv.mx_map(B, H, H, C, DEV)
    yv.quant_mxfp8_map(x.view(B, H, H, C).to(torch.bfloat16).to(DEV), m)
    wq, ws = yv.quant_conv_weight_mxfp8(torch.eye(C, dtype=torch.bfloat16, device=DEV))
    out = torch.zeros(B, H, H, C, dtype=torch.bfloat16, device=DEV) if bf16_out else None
    out_mx = yv.mx_map(B, H, H, C, DEV)
    yv.conv2d_mxfp8(yv.mx_view(m, 0, C), None, B, H, H, 1, 1, wq, ws, torch.zeros(C, device=DEV), out, 0, 0, out_mx=out_mx)
    torch.cuda.synchronize()
    assert torch.equal(out_mx[0].cpu().view(-1, C), qb) and torch.equal(out_mx[1].cpu().view(-1, C // 32), sb)
    if bf16_out:
        assert torch.equal(out.cpu().float().view(-1, C), x)


def test_yolo_engine_rejects_unknown_dtype(yv):
    from yvhip import engines
    sd = engines.init_yolo_state("n", 5, seed=1)
    with pytest.raises(yv.YvError):
        engines.YoloEngine(sd, "n", 5, 128, DEV, dtype="fp8")


# Gates from the MI355X measurement of the shipped plans (B = 2, 640 x 640, seeded random weights; the test prints its values):
# rel-L2 of the logits (max over the six per-scale tensors) with ~50 % margin over what plans at least this wide measured
# (n 0.046, s 0.064, m 0.043, tools/mx_plan_accuracy.py); the smallest per-anchor cosine must stay >= 0.99 on every scale.
ENGINE_GATES = {"n": 0.07, "s": 0.09, "m": 0.07}


@pytest.mark.parametrize("scale", ["n", "s", "m"])
def test_yolo_engine_mxfp8_tracks_bf16(yv, scale):
    """YoloEngine(dtype="mxfp8") against the bf16 engine on the same weights and images: per-scale box and class logits."""
    from yvhip import engines
    sd = engines.init_yolo_state(scale, 5, seed=7, head_gain=4.0)
    e16 = engines.YoloEngine(sd, scale, 5, 640, DEV)
    e8 = engines.YoloEngine(sd, scale, 5, 640, DEV, dtype="mxfp8")
    assert e8.mx_layers == engines.mx_conv_plan(scale, 5) and len(e8.mx_layers) > 0 and e16.mx_layers == []
    g = torch.Generator().manual_seed(8)
    img = torch.randint(0, 256, (2, 640, 640, 3), generator=g, dtype=torch.uint8).to(DEV)
    b16, c16 = e16.forward_raw(img)
    b8, c8 = e8.forward_raw(img)
    torch.cuda.synchronize()
    rel_max, cos_min = 0.0, 1.0
    for part16, part8 in ((b16, b8), (c16, c8)):
        for a, b in zip(part16, part8):
            a, b = a.double().flatten(0, 2), b.double().flatten(0, 2)            # (anchors, channels)
            rel_max = max(rel_max, float((b - a).norm() / a.norm()))
            cos_min = min(cos_min, float(F.cosine_similarity(a, b, dim=1).min()))
    print(f"\nYOLOv8{scale} mxfp8 vs bf16: {len(e8.mx_layers)} MX convolutions, logits rel-L2 max {rel_max:.4f} "
          f"(gate {ENGINE_GATES[scale]}), per-anchor cosine min {cos_min:.5f} (gate 0.99)")
    assert rel_max < ENGINE_GATES[scale] and cos_min >= 0.99


def _mx_pipeline():
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    name, S = "vit_tiny_test", 128
    vit = engines.VitEngine(engines.init_vit_wrapper_state(name, 5, 4), name, 5, device=DEV, dtype="mxfp8")
    det = engines.YoloEngine(engines.init_yolo_state("n", 5, 3, 4.0), "n", 5, S, DEV, dtype="mxfp8")
    assert det.mx_layers
    return DetectClassifyPipeline(det, [vit], max_crops_per_image=3), S


def test_pipeline_with_mxfp8_detector_and_classifier(yv):
    """Pipelined two-stream / split schedules with an MXFP8 detector and an MXFP8 classifier give bitwise the
    single-stream results."""
    from yvhip.pipeline import PipelinedRunner
    pipe, S = _mx_pipeline()
    g = torch.Generator().manual_seed(43)
    batches = [torch.randint(0, 256, (4, S, S, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(4)]
    keys = ("det_count", "det_box", "det_score", "crop_list", "crop_total", "cls_logits", "cls_label")
    ref = []
    for im in batches:
        o = pipe(im)
        torch.cuda.synchronize()
        ref.append({k: o[k].clone() for k in keys})
    assert any(int(r["crop_total"][0]) > 0 for r in ref)
    for split in (False, True):
        runner = PipelinedRunner(pipe, split_classifier=split)
        outs = [runner.submit(im) for im in batches]
        runner.sync()
        for o, r in zip(outs, ref):
            for k in keys:
                assert torch.equal(o[k], r[k]), (split, k)


def test_mxfp8_detector_step_is_graph_capturable(yv):
    """The MXFP8 detector's step allocates nothing and never waits on the host: captured into a graph and replayed on new
    images it gives the eager step's results."""
    pipe, S = _mx_pipeline()
    g = torch.Generator().manual_seed(33)
    batches = [torch.randint(0, 256, (4, S, S, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(3)]
    keys = ("det_count", "det_box", "crop_list", "crop_total", "cls_logits", "cls_label")
    ref = []
    for im in batches:
        o = pipe(im)
        torch.cuda.synchronize()
        ref.append({k: o[k].clone() for k in keys})
    static = batches[0].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe(static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pipe(static)
    for im, r in zip(batches, ref):
        static.copy_(im)
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(out[k], r[k]), k


def test_trt_module_mxfp8(yv):
    from YOLOTensorRT.models import TRTModule
    m = TRTModule("random:m", dtype="mxfp8")
    assert m.engine.mx_layers
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, 256, (2, 640, 640, 3), generator=g, dtype=torch.uint8).to(DEV)
    num, boxes, scores, labels = m(x)
    torch.cuda.synchronize()
    assert num.shape == (2, 1) and boxes.shape == (2, 100, 4) and scores.shape == (2, 100) and labels.shape == (2, 100)
