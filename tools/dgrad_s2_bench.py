"""Data gradient of the detector trainer's stride-2 convolutions, two launch sequences per layer of YOLOv8s and YOLOv8n at
16 x 640 x 640 (model.1, 3, 5, 7, 16, 19: the shapes of yolo_s2_dgrad_shapes, i.e. what bench.py --mode train-yolo runs):

  A  yv_conv_weight_dgrad, yv_view_op(zero insertion), yv_conv2d_ws (3 x 3 / stride 1 over the grid four times dz's size)
                                                                                                  - YoloTrainer's default
  B  yv_conv_weight_dgrad, yv_conv2d_dgrad_s2 (the four parity phases in one launch)              - YoloTrainer(phase_dgrad=True)

Both accumulate into dx (res = dx), as the trainer does.  One process; per shape the arms alternate round by round until each has
at least MIN_SECONDS of timed launches (device events around INNER back-to-back sequences per round), the median round is
reported.  The parts (weight flip | zero insertion | convolution | phase launch) are timed the same way for a fifth of that
time: they say where an arm gains or loses, they do not add up to the sequence exactly.  Nothing is flushed between launches.
--split adds arm S: B with one launch per phase (option "dgrad_s2_split").  Layers the entry rejects are listed without arm B.

  python tools/dgrad_s2_bench.py [--split] [--out FILE]"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolov8-vit_amd"))
import torch
import yvhip
from yvhip.yolo_training import yolo_s2_dgrad_shapes

DEV, MIN_SECONDS, ROUND_MS = "cuda:0", 0.5, 20.0
SIZE, BATCH = 640, 16


class Layer:
    """Operands of one data gradient: N(0, 1) dz and dx, N(0, 1 / K) weights (timing does not depend on the values)."""

    def __init__(self, hin, cin, cout, g):
        self.hin, self.hout, self.cin, self.cout = hin, hin // 2, cin, cout
        self.w = (torch.randn(cout, 9 * cin, generator=g, device=DEV) / math.sqrt(9 * cout)).to(torch.bfloat16)
        self.wd = torch.zeros(cin, 9 * cout, dtype=torch.bfloat16, device=DEV)
        self.dz = torch.randn(BATCH * self.hout * self.hout, cout, generator=g, device=DEV).to(torch.bfloat16)
        self.zi = torch.zeros(BATCH * hin * hin, cout, dtype=torch.bfloat16, device=DEV)
        self.dx = torch.randn(BATCH * hin * hin, cin, generator=g, device=DEV).to(torch.bfloat16)
        self.dzv, self.ziv, self.dxv = yvhip.mview(self.dz), yvhip.mview(self.zi), yvhip.mview(self.dx)
        self.route_a = yvhip.conv2d_instance(BATCH, hin, hin, 3, 1, cout, 0, cin, cin, cin, yvhip.EPI_RES_BF16)
        try:
            self.route_b = yvhip.conv_dgrad_s2_route(BATCH, hin, hin, 3, cin, cout)
        except yvhip.YvError:
            self.route_b = None

    def flip(self):
        yvhip.conv_weight_dgrad(self.w, self.cout, 9, self.cin, self.wd)

    def insert(self):
        yvhip.view_op(yvhip.VIEW_ZERO_INSERT, self.dzv, self.ziv, BATCH, self.hout, self.hout)

    def conv(self):
        yvhip.conv_view(self.ziv, BATCH, self.hin, self.hin, 3, 1, self.wd, self.cin, self.dxv, res=self.dxv)

    def phase(self):
        yvhip.conv_dgrad_s2(self.dzv, BATCH, self.hout, self.hout, self.wd, self.cin, self.cout, self.dxv, res=self.dxv)

    def arm_a(self):
        self.flip(); self.insert(); self.conv()

    def arm_b(self):
        self.flip(); self.phase()

    def arm_s(self):
        yvhip.set_option("dgrad_s2_split", 1)
        try:
            self.arm_b()
        finally:
            yvhip.set_option("dgrad_s2_split", 0)


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


def table(out, split):
    g = torch.Generator(device=DEV).manual_seed(0)
    lines = [f"# python tools/dgrad_s2_bench.py{' --split' if split else ''}   ({torch.cuda.get_device_name(0)}; {BATCH} x {SIZE} x {SIZE}; us per sequence, "
             f"median of alternating rounds, >= {MIN_SECONDS} s of launches per arm; route A: yv_conv2d_instance, B: yv_conv2d_dgrad_s2_route "
             f"kernel / staged / use)",
             f"{'layer':14s} {'cin':>4s} {'cout':>4s} {'hin':>4s} {'rows/phase':>10s} {'A':>3s} {'B':>7s} | {'A us':>8s} {'B us':>8s} {'B - A':>8s} "
             f"{'B / A':>6s}" + (f" {'S us':>8s}" if split else "") + f" | {'flip':>6s} {'insert':>7s} {'conv':>8s} {'phase':>8s}"]
    print("\n".join(lines), flush=True)
    for scale in ("s", "n"):
        tot = dict(a=0.0, b=0.0, s=0.0)
        for key, hin, cin, cout in yolo_s2_dgrad_shapes(scale, SIZE):
            la = Layer(hin, cin, cout, g)
            name, rows, rb = f"v8{scale} {key}", BATCH * la.hout * la.hout, la.route_b
            if rb is None:
                (a,), rounds, inner = alternate([la.arm_a], MIN_SECONDS)
                lines.append(f"{name:14s} {cin:4d} {cout:4d} {hin:4d} {rows:10d} {la.route_a:3d} {'-':>7s} | {a:8.1f}   (not eligible: stays on A)")
                print(lines[-1], flush=True)
                continue
            arms = [la.arm_a, la.arm_b] + ([la.arm_s] if split else [])
            t, rounds, inner = alternate(arms, MIN_SECONDS)
            (pf, pi, pc, pp), _, _ = alternate([la.flip, la.insert, la.conv, la.phase], MIN_SECONDS / 5)
            a, b = t[0], t[1]
            lines.append(f"{name:14s} {cin:4d} {cout:4d} {hin:4d} {rows:10d} {la.route_a:3d} {rb.kernel:2d}/{int(rb.staged)}/{int(rb.use)}   | {a:8.1f} {b:8.1f} "
                         f"{b - a:+8.1f} {b / a:6.3f}" + (f" {t[2]:8.1f}" if split else "") + f" | {pf:6.1f} {pi:7.1f} {pc:8.1f} {pp:8.1f}")
            print(lines[-1] + f"   ({rounds} rounds of {inner})", flush=True)
            tot["a"] += a; tot["b"] += b; tot["s"] += t[2] if split else 0.0
            del la
        lines.append(f"  YOLOv8{scale}, eligible layers (us): A {tot['a']:.0f}, B {tot['b']:.0f}, B - A {tot['b'] - tot['a']:+.0f}"
                     + (f", one launch per phase {tot['s']:.0f}" if split else ""))
        print(lines[-1], flush=True)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    yvhip.require_gpu()
    argv = sys.argv[1:]
    table(argv[argv.index("--out") + 1] if "--out" in argv else None, "--split" in argv)
