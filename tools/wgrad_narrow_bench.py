"""Weight gradients of the detector, 128 x 128 tiles (gemm_tn_kernel) against the tile wgrad_route picks (gemm_tn_narrow_kernel,
64 / 32 x 256), kernel plus slice reduce, for every weight-gradient shape of YOLOv8n (nc 5) and YOLOv8s (nc 80) at 16 x 640 x 640
(yvhip.yolo_training.yolo_wgrad_shapes: the 1x1 layers and the im2col path through yv_wgrad_tiled, the 3x3 / stride 1 layers
through yv_wgrad_conv3_tiled on the padded pixel grid).  One process; per shape the two tiles alternate over ROUNDS rounds of
INNER launches after a cache flush, the median round is reported.

  python tools/wgrad_narrow_bench.py [--out FILE]     the table
  python tools/wgrad_narrow_bench.py one              three launches per tile of the model.4 bottleneck shape of YOLOv8s and
                                                      nothing else: the program of a counter run (rocprofv3 --pmc ... -- python ...)"""
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolov8-vit_amd"))
import torch
import yvhip
from yvhip.yolo_training import yolo_wgrad_shapes

DEV, ROUNDS, INNER = "cuda:0", 7, 10


class Shape:
    """Operands of one weight-gradient product: N(0, 1) bf16 (timing does not depend on the values)."""

    def __init__(self, T, N, K, pitch, g):
        self.T, self.N, self.K, self.pitch = T, N, K, pitch
        self.dy = torch.randn(T, N, generator=g, device=DEV).to(torch.bfloat16)
        self.dw = torch.zeros(N, K, device=DEV)
        if pitch:
            cin, mg = K // 9, pitch + 1
            self.buf = torch.randn((T + 2 * mg) * cin, generator=g, device=DEV).to(torch.bfloat16)
            self.x = self.buf[mg * cin:(mg + T) * cin].view(T, cin)
        else:
            self.x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)

    def run(self, tile_n):
        if self.pitch:
            yvhip.wgrad_conv3(self.dy, self.x, self.dw, self.T, self.pitch, tile_n=tile_n)
        else:
            yvhip.wgrad(self.dy, self.x, self.dw, tile_n=tile_n)


def alternate(sh, tiles, flush):
    """Median over ROUNDS of the microseconds per launch of each tile, the tiles alternating inside every round."""
    ts = {t: [] for t in tiles}
    for t in tiles:
        sh.run(t)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for t in tiles:
            flush.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                sh.run(t)
            e1.record()
            torch.cuda.synchronize()
            ts[t].append(e0.elapsed_time(e1) / INNER * 1e3)
    return {t: sorted(v)[ROUNDS // 2] for t, v in ts.items()}, {t: (min(v), max(v)) for t, v in ts.items()}


def table(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    flush = torch.zeros(128 * 1024 * 1024, device=DEV)             # 512 MB: past the 256 MB of last-level cache
    lines = [f"# python tools/wgrad_narrow_bench.py   ({torch.cuda.get_device_name(0)}; us per launch incl. the slice reduce, median of "
             f"{ROUNDS} alternating rounds of {INNER} launches, cache flushed before each round; [min .. max] of the rounds)"]
    for scale, nc in (("n", 5), ("s", 80)):
        count = collections.Counter((T, N, K, p) for _, T, N, K, p in yolo_wgrad_shapes(scale, nc, 640, 16))
        names = {}
        for key, T, N, K, p in yolo_wgrad_shapes(scale, nc, 640, 16):
            names.setdefault((T, N, K, p), key)
        lines.append(f"YOLOv8{scale} nc {nc}, 16 x 640 x 640: {sum(count.values())} weight gradients, {len(count)} shapes")
        lines.append(f"{'first layer of the shape':28s} {'x':>2s} {'T':>8s} {'N':>4s} {'K':>5s} {'path':>6s} | {'128: tiles x S':>14s} {'us':>8s} {'[min .. max]':>17s} |"
                     f" {'routed: tile tiles x S':>22s} {'us':>8s} {'[min .. max]':>17s} | routed / 128")
        tot = collections.defaultdict(float)
        for (T, N, K, p), n in sorted(count.items(), key=lambda kv: (-kv[0][0], kv[0][1], kv[0][2])):
            r0, r = yvhip.wgrad_route(T, N, K, 128), yvhip.wgrad_route(T, N, K, 0)
            sh = Shape(T, N, K, p, g)
            head = f"{names[(T, N, K, p)]:28s} {n:2d} {T:8d} {N:4d} {K:5d} {'conv3' if p else 'matrix':>6s} | {r0.tiles:8d} x {r0.slices:3d}"
            if r.tile_n == 128:
                med, rng = alternate(sh, [128], flush)
                lines.append(f"{head} {med[128]:8.1f} [{rng[128][0]:6.1f} .. {rng[128][1]:6.1f}] | {'128 (the same launch)':>22s}")
                tot["same"] += n * med[128]
            else:
                med, rng = alternate(sh, [128, 0], flush)
                lines.append(f"{head} {med[128]:8.1f} [{rng[128][0]:6.1f} .. {rng[128][1]:6.1f}] | {r.tile_n:12d} {r.tiles:4d} x {r.slices:3d} {med[0]:8.1f} "
                             f"[{rng[0][0]:6.1f} .. {rng[0][1]:6.1f}] | {med[0] / med[128]:6.3f}")
                tot["128"] += n * med[128]
                tot["routed"] += n * med[0]
            del sh
            print(lines[-1], flush=True)
        lines.append(f"  sum over the step's launches (us): shapes the route leaves on 128 x 128: {tot['same']:.0f};  shapes it moves: "
                     f"{tot['128']:.0f} at 128 x 128, {tot['routed']:.0f} routed ({tot['routed'] / max(tot['128'], 1e-9):.3f});  all weight gradients: "
                     f"{tot['same'] + tot['128']:.0f} -> {tot['same'] + tot['routed']:.0f}")
        print(lines[-1], flush=True)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


def one():
    key, T, N, K, p = next(s for s in yolo_wgrad_shapes("s", 80, 640, 16) if s[0] == "model.4.m.0.cv1.conv")
    sh = Shape(T, N, K, p, torch.Generator(device=DEV).manual_seed(0))
    for t in (128, 64, 32):
        for _ in range(3):
            sh.run(t)
    torch.cuda.synchronize()
    print(f"{key}: T {T} N {N} K {K} pitch {p}; routes " + "  ".join(str(yvhip.wgrad_route(T, N, K, t)) for t in (128, 64, 32)))


if __name__ == "__main__":
    yvhip.require_gpu()
    if sys.argv[1:2] == ["one"]:
        one()
    else:
        table(sys.argv[2] if sys.argv[1:2] == ["--out"] else None)
