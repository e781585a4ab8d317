"""BatchNorm batch statistics of the detector trainer's forward, two launch sequences per BatchNorm convolution of YOLOv8s (nc 80)
at 16 x 640 x 640 (the shapes of YoloTrainer.blocks / .geom, i.e. what bench.py --mode train-yolo runs):

  A  yv_conv2d_ws, then yv_bn_stats (a pass over z + the finaliser)                  - YoloTrainer's default
  B  yv_conv2d_stats (the statistics from the convolution's epilogue), then yv_bn_stats_finish   - YoloTrainer(fused_bn_stats=True)

One process; per shape the arms alternate round by round until each has at least MIN_SECONDS of timed launches (device events
around INNER back-to-back sequences per round), the median round is reported.  The parts of each arm (conv | statistics) are
timed the same way for a fifth of that time: they say where an arm gains or loses, they do not add up to the sequence exactly.
Nothing is flushed between launches: as in the training step, z is read right after it was written.

  python tools/conv_stats_bench.py [--out FILE]"""
import collections
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolov8-vit_amd"))
import torch
import yvhip
from yvhip.yolo_training import BN_EPS, BN_MOMENTUM, YoloTrainer, init_yolo_train_state

DEV, MIN_SECONDS, ROUND_MS = "cuda:0", 0.5, 20.0
SCALE, NC, SIZE, BATCH = "s", 80, 640, 16


def trainer_shapes():
    """[(first key, count, cin, cout, k, s, hin, hout)] of the BatchNorm blocks, in the trainer's order of first appearance."""
    tr = YoloTrainer(init_yolo_train_state(SCALE, NC, seed=0), scale=SCALE, nc=NC, size=SIZE, batch=BATCH)
    count, first = collections.Counter(), {}
    for b in tr.blocks:
        hin, hout = tr.geom[b.key]
        if b.bn:
            sh = (b.cin, b.cout, b.k, b.s, hin, hout)
            count[sh] += 1
            first.setdefault(sh, b.key)
    del tr
    torch.cuda.empty_cache()
    return [(first[sh], n) + sh for sh, n in count.items()]


class Layer:
    """Operands of one BatchNorm convolution: N(0, 1) input, N(0, 1 / K) weights (timing does not depend on the values)."""

    def __init__(self, cin, cout, k, s, hin, hout, g):
        self.args = (BATCH, hout, hout, k, s)
        self.T, self.C = BATCH * hout * hout, cout
        self.x = torch.randn(BATCH, hin, hin, cin, generator=g, device=DEV).to(torch.bfloat16)
        self.w = (torch.randn(cout, k * k * cin, generator=g, device=DEV) / math.sqrt(k * k * cin)).to(torch.bfloat16)
        self.z = torch.zeros(self.T, cout, dtype=torch.bfloat16, device=DEV)
        self.ws = torch.zeros(max(yvhip.bn_ws_floats(self.T, cout), yvhip.conv_stats_ws_floats(self.T, cout)), device=DEV)
        self.st = [torch.zeros(cout, device=DEV) for _ in range(4)]                   # mean, rstd, run_mean, run_var
        self.xv, self.zv = yvhip.mview(self.x), yvhip.mview(self.z)
        self.route = yvhip.conv2d_instance(BATCH, hout, hout, k, s, cin, 0, cout, cout, ws_bytes=0)

    def conv(self):
        yvhip.conv_view(self.xv, *self.args, self.w, self.C, self.zv)

    def stats(self):
        yvhip.bn_stats(self.zv, self.T, *self.st, self.ws, BN_EPS, BN_MOMENTUM)

    def conv_stats(self):
        yvhip.conv_view_stats(self.xv, *self.args, self.w, self.C, self.zv, self.ws)

    def finish(self):
        yvhip.bn_stats_finish(self.ws, self.T, *self.st, BN_EPS, BN_MOMENTUM)

    def arm_a(self):
        self.conv(); self.stats()

    def arm_b(self):
        self.conv_stats(); self.finish()


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


def table(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    lines = [f"# python tools/conv_stats_bench.py   ({torch.cuda.get_device_name(0)}; YOLOv8{SCALE} nc {NC}, {BATCH} x {SIZE} x {SIZE}; us per "
             f"sequence, median of alternating rounds, >= {MIN_SECONDS} s of launches per arm; route: yv_conv2d_instance without split-K)",
             f"{'first layer of the shape':26s} {'x':>2s} {'k/s':>3s} {'cin':>4s} {'cout':>4s} {'hout':>4s} {'T':>8s} {'tiles':>6s} {'route':>5s} |"
             f" {'A us':>8s} {'B us':>8s} {'B - A':>8s} {'B / A':>6s} | {'conv_ws':>8s} {'bn_stats':>8s} | {'conv_stats':>10s} {'finish':>8s}"]
    print("\n".join(lines), flush=True)
    tot = collections.defaultdict(float)
    by_route = collections.defaultdict(lambda: [0.0, 0.0])
    shapes = trainer_shapes()
    for key, n, cin, cout, k, s, hin, hout in shapes:
        la = Layer(cin, cout, k, s, hin, hout, g)
        (a, b), rounds, inner = alternate([la.arm_a, la.arm_b], MIN_SECONDS)
        (pc, ps, pcs, pf), _, _ = alternate([la.conv, la.stats, la.conv_stats, la.finish], MIN_SECONDS / 5)
        lines.append(f"{key:26s} {n:2d} {k}/{s} {cin:4d} {cout:4d} {hout:4d} {la.T:8d} {(la.T + 127) // 128:6d} {la.route:5d} |"
                     f" {a:8.1f} {b:8.1f} {b - a:+8.1f} {b / a:6.3f} | {pc:8.1f} {ps:8.1f} | {pcs:10.1f} {pf:8.1f}")
        print(lines[-1] + f"   ({rounds} rounds of {inner})", flush=True)
        tot["a"] += n * a; tot["b"] += n * b
        tot["saved"] += n * max(a - b, 0.0); tot["lost"] += n * max(b - a, 0.0)
        by_route[la.route][0] += n * a; by_route[la.route][1] += n * b
        del la
    lines.append(f"  sum over the step's {sum(sh[1] for sh in shapes)} BatchNorm convolutions (us): A {tot['a']:.0f}, B {tot['b']:.0f}, "
                 f"B - A {tot['b'] - tot['a']:+.0f} (saved {tot['saved']:.0f} on the shapes that win, lost {tot['lost']:.0f} on those that lose)")
    for r, (a, b) in sorted(by_route.items()):
        lines.append(f"  route {r:2d}: A {a:8.0f}  B {b:8.0f}  B - A {b - a:+8.0f}")
    print("\n".join(lines[-1 - len(by_route):]), flush=True)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    yvhip.require_gpu()
    table(sys.argv[2] if sys.argv[1:2] == ["--out"] else None)
