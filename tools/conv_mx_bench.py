#!/usr/bin/env python3
"""Per-layer A/B of the detector convolutions: the bf16 kernel yv_conv2d picks against the MXFP8 kernel (yv_conv2d_mxfp8) on
every convolution of mx_conv_plan (before any speed filter) for YOLOv8m at batch 64 and YOLOv8n at batch 32 (640 x 640).
Dense inputs (pixel stride = Cin), bias + SiLU; the bf16 launch writes the bf16 output, the MX launch writes the bf16
output AND the MX-map output (what the engine's MX layers write when an MX convolution reads their output).  Not in these
per-layer figures: the yv_quant_mxfp8_map passes the engine adds behind bf16-only producers (stem, fused C2f, SPPF) - they
are in the detect-stage figures of tools/large_mx_e2e.py.
  python tools/conv_mx_bench.py                      device events around REPS back-to-back launches per layer and kernel
  rocprofv3 --kernel-trace --stats -d DIR -o conv_mx --output-format csv -- python tools/conv_mx_bench.py
  python tools/conv_mx_bench.py --trace DIR/.../conv_mx_kernel_trace.csv
                                                     the same table from the kernel trace (dispatch durations; each layer's
                                                     launches sit between the fill / quantisation kernels of its set-up)"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch

from yvhip import engines

REPS, WARM = int(os.environ.get("REPS", 20)), 3
dev = "cuda:0"
CONV_KERNELS = ("igemm_kernel", "cgemm_dma_kernel", "splitk_reduce_kernel", "cgemm_mx_kernel")


def layer_shapes(scale, nc=5):
    plan = set(engines.mx_conv_plan(scale, nc, speed_filter=False, min_width=0))
    for e in engines.detect_launches(scale, nc):
        if isinstance(e, engines.Conv) and e.key in plan:
            yield e.key, [(c, up) for _, _, c, up in e.srcs], e.k, e.stride, e.cout, 640 // e.down


def time_it(fn):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def all_layers():
    for scale, B in (("m", 64), ("n", 32)):
        for key, srcs, k, st, co, H in layer_shapes(scale):
            yield scale, B, key, srcs, k, st, co, H


def kind(k, st, srcs):
    cin = sum(c for c, _ in srcs)
    return f"{k}x{k}/s{st} Cin%128{'=0' if cin % 128 == 0 else '!=0'}"


def report(times):
    """times: list of (bf16 us, mx us) in all_layers() order."""
    tot = {}
    by_kind = {}
    last = None
    for (scale, B, key, srcs, k, st, co, H), (t16, t8) in zip(all_layers(), times):
        if scale != last:
            print(f"YOLOv8{scale}, batch {B}")
            print(f"{'layer':28s} {'k/s':>4s} {'Cin':>5s} {'Cout':>5s} {'H':>4s} {'GFLOP':>7s} {'bf16 us':>8s} {'mx us':>8s} "
                  f"{'bf16 TF/s':>9s} {'mx TF/s':>8s} {'inst':>4s}")
            last = scale
        cin = sum(c for c, _ in srcs)
        fl = 2.0 * B * H * H * co * k * k * cin
        import yvhip
        inst = yvhip.conv2d_mxfp8_instance(B, H, H, k, st, cin, co)
        print(f"{key:28s} {k}/{st:<2d} {cin:5d} {co:5d} {H:4d} {fl / 1e9:7.1f} {t16:8.1f} {t8:8.1f} {fl / t16 / 1e6:9.1f} "
              f"{fl / t8 / 1e6:8.1f} {inst:4d}")
        a = tot.setdefault(scale, [0.0, 0.0]); a[0] += t16; a[1] += t8
        b = by_kind.setdefault((scale, kind(k, st, srcs)), [0.0, 0.0, 0]); b[0] += t16; b[1] += t8; b[2] += 1
    for scale, (a, b) in tot.items():
        print(f"YOLOv8{scale} MX-eligible layers: bf16 {a:.0f} us, mx {b:.0f} us")
    for (scale, kd), (a, b, n) in sorted(by_kind.items()):
        print(f"YOLOv8{scale} kind {kd:22s} layers {n:3d}: bf16 {a:8.0f} us, mx {b:8.0f} us ({(b / a - 1) * 100:+.1f} %)")


def from_trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    segs, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        conv = any(c in name for c in CONV_KERNELS)
        if not conv:
            if cur:
                segs.append(cur)
            cur = None
            continue
        cur = cur or [0.0, 0.0]
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        cur[1 if "cgemm_mx_kernel" in name else 0] += d
    if cur:
        segs.append(cur)
    n = WARM + REPS
    times = [(a / n, b / n) for a, b in segs]
    layers = list(all_layers())
    assert len(times) == len(layers), (len(times), len(layers))
    report(times)


def run():
    import yvhip
    times = []
    for scale, B, key, srcs, k, st, co, H in all_layers():
        g = torch.Generator().manual_seed(len(key))
        ins16, insmx, keep = [], [], []
        for c, up in srcs:
            h = (H * st) >> up
            x = (torch.randn(B, h, h, c, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            m = yvhip.mx_map(B, h, h, c, dev)
            yvhip.quant_mxfp8_map(x, m)
            keep += [x, m]
            ins16.append(yvhip.view(x, 0, c, up))
            insmx.append(yvhip.mx_view(m, 0, c, up))
        cin = sum(c for c, _ in srcs)
        w = (torch.randn(co, k * k * cin, generator=g) * (2.0 / (k * k * cin)) ** 0.5).to(torch.bfloat16).to(dev)
        bias = torch.zeros(co, device=dev)
        wq, ws = yvhip.quant_conv_weight_mxfp8(w)
        out = torch.empty(B, H, H, co, dtype=torch.bfloat16, device=dev)
        out_mx = yvhip.mx_map(B, H, H, co, dev)
        torch.cuda.synchronize()
        i1 = ins16[1] if len(ins16) > 1 else None
        m1 = insmx[1] if len(insmx) > 1 else None
        t16 = time_it(lambda: yvhip.conv2d(ins16[0], i1, B, H, H, k, st, w, bias, out, 0, yvhip.EPI_SILU))
        t8 = time_it(lambda: yvhip.conv2d_mxfp8(insmx[0], m1, B, H, H, k, st, wq, ws, bias, out, 0, yvhip.EPI_SILU,
                                                out_mx=out_mx))
        times.append((t16, t8))
        del keep, ins16, insmx
    report(times)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        from_trace(sys.argv[2])
    else:
        run()
