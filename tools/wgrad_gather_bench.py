"""Weight gradient of the detector trainer's 3 x 3 / stride-2 convolutions, two launch sequences per layer of YOLOv8s and YOLOv8n
at 16 x 640 x 640 (model.0, 1, 3, 5, 7, 16, 19: what bench.py --mode train-yolo runs):

  A  yv_im2col3 into the (T, 9 * Cin) scratch, yv_wgrad(_tiled) on it           - YoloTrainer's default for these layers
  B  yv_wgrad_conv3_gather on dz and x themselves                                - YoloTrainer(gather_wgrad=True)

Both with the same N tile, hence the same route (tiles, token slices): tile 128 is what the default trainer passes, tile 0 (the
tile yv_wgrad_route picks) what YoloTrainer(narrow_wgrad=True) passes.  One process; per layer and tile the arms alternate round by
round until each has at least MIN_SECONDS of timed launches (device events around INNER back-to-back sequences per round, after
a warm-up of every arm), the median round is reported.  The im2col launch alone is timed the same way for a fifth of that time.
Nothing is flushed between launches.  "use" is what yv_wgrad_conv3_gather_route answers for the layer.

  python tools/wgrad_gather_bench.py [--out FILE]"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolov8-vit_amd"))
import torch
import yvhip
from yvhip.yolo_training import Block, train_launches

DEV, MIN_SECONDS, ROUND_MS = "cuda:0", 0.5, 20.0
SIZE, BATCH = 640, 16


class Layer:
    """Operands of one weight gradient: N(0, 1) dz and x (timing does not depend on the values)."""

    def __init__(self, hin, cin, cout, g):
        self.hin, self.hout, self.cin, self.cout = hin, hin // 2, cin, cout
        self.T = BATCH * self.hout * self.hout
        assert self.T % 64 == 0
        self.x = torch.randn(BATCH * hin * hin, cin, generator=g, device=DEV).to(torch.bfloat16)
        self.dz = torch.randn(self.T, cout, generator=g, device=DEV).to(torch.bfloat16)
        self.col = torch.zeros(self.T, 9 * cin, dtype=torch.bfloat16, device=DEV)
        self.dw = torch.zeros(cout, 9 * cin, device=DEV)
        self.xv = yvhip.mview(self.x)

    def im2col(self):
        yvhip.im2col3(self.xv, BATCH, self.hin, self.hin, 2, self.col)

    def arm_a(self, tile):
        self.im2col()
        yvhip.wgrad(self.dz, self.col, self.dw, T=self.T, tile_n=tile)

    def arm_b(self, tile):
        yvhip.wgrad_conv3_gather(self.dz, self.xv, self.dw, BATCH, self.hin, self.hin, 2, tile_n=tile)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3                                         # us per call


def alternate(fns, seconds):
    """Median microseconds per call of each function, the functions alternating inside every round."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    est = max(timed(f, 3) for f in fns)
    inner = int(min(max(ROUND_MS * 1e3 / est, 3), 400))
    rounds = max(5, int(math.ceil(seconds * 1e6 / (inner * est)))) | 1
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            ts[i].append(timed(f, inner))
    return [sorted(v)[len(v) // 2] for v in ts], rounds, inner


def s2_layers(scale):
    return [(e.key, SIZE // e.down_in, e.cin, e.cout) for e in train_launches(scale, 80)
            if isinstance(e, Block) and e.k == 3 and e.stride == 2]


def table(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    lines = [f"# python tools/wgrad_gather_bench.py   ({torch.cuda.get_device_name(0)}; {BATCH} x {SIZE} x {SIZE}; us per sequence, median of "
             f"alternating rounds, >= {MIN_SECONDS} s of launches per arm; A: im2col3 + wgrad, B: wgrad_conv3_gather; route: N tile x "
             f"K tile, tiles, slices)",
             f"{'layer':14s} {'cin':>4s} {'cout':>4s} {'hin':>4s} {'T':>8s} {'tile_n':>6s} {'route':>16s} {'use':>3s} | {'A us':>8s} {'B us':>8s} "
             f"{'B - A':>8s} {'B / A':>6s} | {'im2col':>8s}"]
    print("\n".join(lines), flush=True)
    for scale in ("s", "n"):
        tot = {128: [0.0, 0.0], 0: [0.0, 0.0]}
        for key, hin, cin, cout in s2_layers(scale):
            la = Layer(hin, cin, cout, g)
            (pi,), _, _ = alternate([la.im2col], MIN_SECONDS / 5)
            for tile in (128, 0):
                r, use = yvhip.wgrad_conv3_gather_route(BATCH, hin, hin, 2, cin, cout, tile)
                (a, b), rounds, inner = alternate([lambda: la.arm_a(tile), lambda: la.arm_b(tile)], MIN_SECONDS)
                lines.append(f"{'v8' + scale + ' ' + key:14s} {cin:4d} {cout:4d} {hin:4d} {la.T:8d} {tile:6d} "
                             f"{f'{r.tile_n}x{r.tile_k} {r.tiles}t {r.slices}s':>16s} {int(use):3d} | {a:8.1f} {b:8.1f} {b - a:+8.1f} {b / a:6.3f} | {pi:8.1f}")
                print(lines[-1] + f"   ({rounds} rounds of {inner})", flush=True)
                tot[tile][0] += a; tot[tile][1] += b
            del la
        for tile in (128, 0):
            a, b = tot[tile]
            lines.append(f"  YOLOv8{scale}, tile_n {tile}, seven layers (us): A {a:.0f}, B {b:.0f}, B - A {b - a:+.0f}")
            print(lines[-1], flush=True)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    yvhip.require_gpu()
    argv = sys.argv[1:]
    table(argv[argv.index("--out") + 1] if "--out" in argv else None)
