#!/usr/bin/env python3
"""Dev tool (GPU box): every grouped launch of the Detect head (YoloEngine(grouped_head=True)) against the
sum of its members' single launches, for YOLOv8n and YOLOv8s (nc 5) at 1, 2, 4 and 32 images of 640 x 640 and one image of
384 x 640, with small_maps off and on ("conv_small" = 0 / engines.SMALL_MAP_PIXELS).
Per step of the head (the three det{s}.0, the six .1; nc 5 has the fused tail, so no .2 step) yvhip.conv2d_group_plan gives the
partition; each launch of two or more members is timed as one conv2d_group call of exactly those members, and each of its
members as its own conv2d call, on the engine's views (channel offsets, pixel strides) and flags.
By the method of tools/conv_small_bench.py: kernel times from the launch's own dispatch packet (yv_set_launch_timing), every
launch of a series on another copy of the weights (CGB_COPIES, default 12), grouped and single series interleaved, median of the
launches of CGB_ROUNDS rounds.  "max single": the longest member alone - the floor of a grouped launch that overlaps perfectly.
The last lines give, per configuration, the head's kernel time grouped (grouped launches + the members left single) against
ungrouped (every member single) and the launches of the head."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip
from yvhip import engines

dev = "cuda:0"
COPIES = int(os.environ.get("CGB_COPIES", 12))
ROUNDS = int(os.environ.get("CGB_ROUNDS", 3))
NC = 5
EXTENTS = [(1, 640, 640), (2, 640, 640), (4, 640, 640), (32, 640, 640), (1, 384, 640)]
NAMES = {yvhip.CONV_DMA_64_3: "dma64x3", yvhip.CONV_SMALL_64: "small64", yvhip.CONV_SMALL_32: "small32", yvhip.CONV_DMA_128_2: "dma128x2"}
g = torch.Generator(device=dev).manual_seed(0)


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


def main():
    old = yvhip.get_option("conv_small")
    print(f"# {torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} x {2 * COPIES} launches, grouped and single series interleaved")
    print(f"# {'net':3s} {'B':>2s} {'extent':>7s} {'small_maps':>10s} {'step':>4s} {'instance':>8s} {'members':>7s} {'grid':>5s}  "
          f"{'grouped':>8s} {'sum single':>10s} {'max single':>10s}  {'grouped / sum':>13s}  members (us alone)")
    totals = []
    try:
        for scale in ("n", "s"):
            ch, c2, c3, _ = engines.detect_widths(scale, NC)
            groups = [e.convs for e in engines.detect_launches(scale, NC, True, False, True) if type(e) is engines.ConvGroup]
            width = {f"out{i}": ch[s] for s, i in enumerate((15, 18, 21))}
            for s in range(3):
                width[f"det{s}.hb"] = width[f"det{s}.hc"] = c2 + c3
            for B, H, W in EXTENTS:
                for small in (0, engines.SMALL_MAP_PIXELS):
                    yvhip.set_option("conv_small", small)
                    bufs = {}
                    for cs in groups:
                        for c in cs:
                            for name, d in ((c.srcs[0][0], c.down), (c.out, c.down)):
                                if name not in bufs:
                                    bufs[name] = torch.randn(B, H // d, W // d, width[name], generator=g, device=dev).to(torch.bfloat16)
                    t_grouped = t_single = 0.0
                    n_launches = n_members = 0
                    for step, cs in enumerate(groups):
                        shapes = [(B, H // c.down, W // c.down, c.k, c.stride, c.srcs[0][2], 0, c.cout, width[c.out], 0, c.flags) for c in cs]
                        n, plan = yvhip.conv2d_group_plan(shapes)
                        n_launches += n
                        n_members += len(cs)
                        ws = [[(torch.randn(c.cout, c.k * c.k * c.srcs[0][2], generator=g, device=dev) * (c.k * c.k * c.srcs[0][2]) ** -0.5)
                               .to(torch.bfloat16) for _ in range(COPIES)] for c in cs]
                        bias = [torch.randn(c.cout, generator=g, device=dev) for c in cs]

                        def member(j, i):
                            c = cs[j]
                            b, off, cc, up = c.srcs[0]
                            return (yvhip.view(bufs[b], off, cc, up), None, B, H // c.down, W // c.down, c.k, c.stride, ws[j][i % COPIES],
                                    bias[j], bufs[c.out], c.out_off, c.flags)
                        singles = {j: [] for j in range(len(cs))}
                        by_launch = {}
                        for j, p in enumerate(plan):
                            by_launch.setdefault(p["launch"], []).append(j)
                        grouped = {l: [] for l, js in by_launch.items() if len(js) > 1}
                        for rd in range(ROUNDS):
                            for l in grouped:
                                js = sorted(by_launch[l], key=lambda j: plan[j]["position"])
                                grouped[l] += timed(lambda i: yvhip.conv2d_group([member(j, i) for j in js]), 2 * COPIES)
                            for j in singles:
                                singles[j] += timed(lambda i: yvhip.conv2d(*member(j, i)), 2 * COPIES)
                        alone = {j: median(v) if v else float("nan") for j, v in singles.items()}
                        for l, js in sorted(by_launch.items()):
                            code = plan[js[0]]["instance"] & 15
                            if len(js) == 1:
                                t_grouped += alone[js[0]]
                                t_single += alone[js[0]]
                                print(f"  {scale:3s} {B:2d} {H:3d}x{W:3d} {'on' if small else 'off':>10s} {step:4d} {NAMES.get(code, str(code)):>8s} "
                                      f"{1:7d} {'':5s}  {'':8s} {alone[js[0]]:10.1f} {'':10s}  {'single launch':>13s}  {cs[js[0]].key}", flush=True)
                                continue
                            js = sorted(js, key=lambda j: plan[j]["position"])
                            rows = {yvhip.CONV_DMA_64_3: 128, yvhip.CONV_SMALL_64: 64}.get(code, 32)
                            last = js[-1]
                            grid = plan[last]["first_wg"] + -(-shapes[last][0] * shapes[last][1] * shapes[last][2] // rows) * -(-shapes[last][7] // 64)
                            tg, ts = median(grouped[l]), sum(alone[j] for j in js)
                            t_grouped += tg
                            t_single += ts
                            print(f"  {scale:3s} {B:2d} {H:3d}x{W:3d} {'on' if small else 'off':>10s} {step:4d} {NAMES.get(code, str(code)):>8s} "
                                  f"{len(js):7d} {grid:5d}  {tg:8.1f} {ts:10.1f} {max(alone[j] for j in js):10.1f}  {tg / ts:13.2f}  "
                                  + " ".join(f"{cs[j].key.replace('model.22.', '')}({alone[j]:.1f})" for j in js), flush=True)
                        del ws
                    totals.append((scale, B, H, W, small, t_grouped, t_single, n_launches, n_members))
                    del bufs
    finally:
        yvhip.set_option("conv_small", old)
    print("#")
    print("# the head's kernel time per configuration: grouped launches + members left single, against every member single")
    for scale, B, H, W, small, tg, ts, nl, nm in totals:
        print(f"#   {scale} B {B:2d} {H}x{W} small_maps {'on ' if small else 'off'}: {tg:7.1f} us in {nl} launches against {ts:7.1f} us in {nm} launches"
              f"  (x {tg / ts:.2f}; {ts - tg:+.1f} us of kernel time, {nm - nl} launches fewer)")


if __name__ == "__main__":
    main()
