#!/usr/bin/env python3
"""Dev tool (GPU box): every layer of engines.dma32_layers - YOLOv8m at 64, 4 and 1 images of 640 x 640, YOLOv8s and YOLOv8n at
32 - on the parent's route and on each instance of cgemm_dma32_kernel, interleaved in one process:
  parent  "conv_dma32" = 0: igemm_kernel;
  d64     cgemm_dma32_kernel<64, 4, 1, 3>   ("conv_dma32_cols" = 64);
  d128    cgemm_dma32_kernel<128, 2, 2, 2>  ("conv_dma32_cols" = 128).
(profiles/conv_dma32_layers.txt also holds the table of the measurement build, which had a 96-wide instance with two and with
three stages behind "conv_dma32_cols" = 96 and a stage option: fastest on no layer, hence deleted.)
By the method of tools/conv_small_bench.py: kernel times from the launch's own dispatch packet (yv_set_launch_timing), every
launch of a series on another copy of its weights (CDB_COPIES, default 12), median of the launches of CDB_ROUNDS interleaved
rounds.  The engine's own views (channel offsets, pixel strides, shortcut) and flags; layers of one class (same shapes and
strides, another slice of the same buffer) are timed once and counted.  "rule": the instance the shipped rule
("conv_dma32" = 1, "conv_dma32_cols" = 0) takes.  The last lines say whether every layer is at least as fast on the rule's
instance as on the parent's route."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip
from yvhip import engines

dev = "cuda:0"
COPIES = int(os.environ.get("CDB_COPIES", 12))
ROUNDS = int(os.environ.get("CDB_ROUNDS", 3))
NC = 80
NETS = [("m", 64), ("m", 4), ("m", 1), ("s", 32), ("n", 32)]
H = W = 640
g = torch.Generator(device=dev).manual_seed(0)
NAMES = {yvhip.CONV_DMA32_64: "d64", yvhip.CONV_DMA32_128: "d128"}


def timed(fn, n):
    recs = []
    fn(0); torch.cuda.synchronize()
    yvhip.reserve_events(2 * n)
    yvhip.CONV_HOOK = lambda M, N, e0, e1: recs.append((e0, e1))
    try:
        for i in range(n):
            fn(i)
    finally:
        yvhip.CONV_HOOK = None
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in recs]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def set_options(opts):
    for k, v in opts.items():
        yvhip.set_option(k, v)


def widths(scale):
    width = {}
    for idx, kind, p in engines.yolo_layers(scale):
        width[f"out{idx}"] = p["cout"]
        if kind == "c2f":
            width[f"y{idx}"], width[f"t{idx}"] = (2 + p["n"]) * (p["cout"] // 2), p["cout"] // 2
        elif kind == "sppf":
            width[f"y{idx}"] = p["cin"] * 2
    _, c2, c3, _ = engines.detect_widths(scale, NC)
    for s in range(3):
        width[f"det{s}.hb"] = width[f"det{s}.hc"] = c2 + c3
    return width


def main():
    off = {"conv_dma32": 0, "conv_dma32_cols": 0}
    routes = {"parent": dict(off), "d64": dict(conv_dma32=1, conv_dma32_cols=64), "d128": dict(conv_dma32=1, conv_dma32_cols=128)}
    names = list(routes)
    print(f"# {torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} x {2 * COPIES} launches, routes interleaved")
    print(f"# {'net':3s} {'B':>2s} {'layer (first of n)':22s} {'n':>2s} {'k':>1s} {'s':>1s} {'cin':>4s} {'cout':>4s} {'M':>7s} {'GFLOP':>6s}  "
          + " ".join(f"{r:>7s}" for r in names) + "  " + " ".join(f"{r + '/p':>7s}" for r in names[1:]) + "  best   rule")
    rows = []
    for scale, B in NETS:
        width = widths(scale)
        set_options(dict(conv_dma32=1, conv_dma32_cols=64))
        keys = set(engines.dma32_layers(scale, NC, B, (H, W)))
        set_options(off)
        seen = {}
        for e in engines.detect_launches(scale, NC):
            if type(e) is not engines.Conv or e.key not in keys:
                continue
            sig = (tuple((width[b], c, up) for b, _, c, up in e.srcs), e.k, e.stride, width[e.out], e.res_off is not None, e.flags,
                   e.cout, e.down)
            if sig in seen:
                seen[sig][1] += 1
            else:
                seen[sig] = [e, 1]
        for e, count in seen.values():
            h, w = H // e.down, W // e.down
            M, ld_out = B * h * w, width[e.out]
            cin = sum(c for _, _, c, _ in e.srcs)
            K = e.k * e.k * cin
            c = [s[2] for s in e.srcs] + [0]
            query = lambda: yvhip.conv2d_instance(B, h, w, e.k, e.stride, c[0], c[1], e.cout, ld_out, ld_out if e.res_off is not None else 0,
                                                  e.flags)
            set_options(dict(conv_dma32=1, conv_dma32_cols=0))
            rule = NAMES.get(query() & 15, "parent")
            set_options(off)
            srcs = []
            for b, coff, ch, up in e.srcs:
                t = torch.randn(B, (h * e.stride) >> up, (w * e.stride) >> up, width[b], generator=g, device=dev).to(torch.bfloat16)
                srcs.append(yvhip.view(t, coff, ch, up))
            ws = [(torch.randn(e.cout, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(COPIES)]
            bias = torch.randn(e.cout, generator=g, device=dev)
            out = torch.zeros(B, h, w, ld_out, dtype=torch.float32 if e.flags & yvhip.EPI_OUT_F32 else torch.bfloat16, device=dev)
            res = out if e.res_off is not None else None
            fn = lambda i: yvhip.conv2d(srcs[0], srcs[1] if len(srcs) > 1 else None, B, h, w, e.k, e.stride, ws[i % COPIES], bias,
                                        out, e.out_off, e.flags, res=res, res_c_off=e.res_off or 0)
            ts = {r: [] for r in routes}
            try:
                for rd in range(ROUNDS):
                    for r, opts in routes.items():
                        set_options(opts)
                        ts[r] += timed(fn, 2 * COPIES)
            finally:
                set_options(off)
            t = {r: median(v) for r, v in ts.items()}
            best = min(names, key=lambda r: t[r])
            rows.append((scale, B, e.key, count, t, best, rule))
            print(f"  {scale:3s} {B:2d} {e.key:22s} {count:2d} {e.k:1d} {e.stride:1d} {cin:4d} {e.cout:4d} {M:7d} {2e-9 * M * K * e.cout:6.2f}  "
                  + " ".join(f"{t[r]:7.1f}" for r in names) + "  " + " ".join(f"{t[r] / t['parent']:7.2f}" for r in names[1:])
                  + f"  {best:6s} {rule}", flush=True)
            del srcs, ws, out
    print("#")
    for scale, B in NETS:
        sub = [x for x in rows if x[0] == scale and x[1] == B]
        s = {r: sum(x[3] * x[4][r] for x in sub) for r in names}
        srule = sum(x[3] * x[4][x[6]] for x in sub)
        print(f"# {scale} at {B:2d}: sum over the pass, us: " + ", ".join(f"{r} {s[r]:.0f}" for r in names) + f"; shipped rule {srule:.0f}")
    taken = [(x, x[4][x[6]] / x[4]["parent"]) for x in rows if x[6] != "parent"]
    slower = [(x[0], x[1], x[2], round(r, 2)) for x, r in taken if r > 1.0]
    print(f"# the shipped rule takes {len(taken)} of {len(rows)} timed layer classes; slower than the parent's route: {len(slower)} {slower if slower else ''}")
    left = [(x[0], x[1], x[2]) + tuple(f"{r} x {x[4][r] / x[4]['parent']:.2f}" for r in names[1:]) for x in rows if x[6] == "parent"]
    print(f"# left on the parent's route: {len(left)} {left if left else ''}")


if __name__ == "__main__":
    main()
