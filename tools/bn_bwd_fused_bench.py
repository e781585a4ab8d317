"""BatchNorm backward sums of the detector trainer, two launch sequences per eligible pair (fused_bn_bwd_pairs: a consumer block's
data gradient writes the whole output gradient da of the producer block that backward() runs next; `use`: what the route answers
for the pair, i.e. whether YoloTrainer(fused_bn_bwd=True) fuses it) of YOLOv8s (nc 80) and YOLOv8n (nc 5)
at 16 x 640 x 640 (the shapes of YoloTrainer.blocks / .geom, i.e. what bench.py --mode train-yolo runs):

  A  yv_conv2d_ws (the data gradient, res = out), then yv_bn_act_bwd (a pass over da and z for the sums, the finaliser, the apply
     pass)                                                                                        - YoloTrainer's default
  B  yv_conv2d_bnbwd (the sums from the data gradient's epilogue), then yv_bn_act_bwd_finish (the finaliser, the apply pass)
                                                                                                  - YoloTrainer(fused_bn_bwd=True)

One process; per shape the arms alternate round by round until each has at least MIN_SECONDS of timed launches (device events
around INNER back-to-back sequences per round); the median round is reported, with the quartile range of arm A's rounds as the
spread of the measurement.  The parts of each arm (data gradient | BatchNorm backward) are timed the same way for a fifth of that
time: they say what the epilogue costs and what the finaliser saves, they do not add up to the sequence exactly.  Nothing is
flushed between launches: as in the training step, da is read right after it was written.  A stride-2 consumer's data gradient
is the stride-1 convolution over its zero-inserted gradient, as the default trainer runs it (the insertion itself is in neither arm).

  python tools/bn_bwd_fused_bench.py [--out FILE]"""
import collections
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolov8-vit_amd"))
import torch
import yvhip
from yvhip.yolo_training import YoloTrainer, fused_bn_bwd_pairs, init_yolo_train_state

DEV, MIN_SECONDS, ROUND_MS = "cuda:0", 0.5, 20.0
MODELS, SIZE, BATCH = (("s", 80), ("n", 5)), 640, 16


def trainer_pairs(scale, nc):
    """[(consumer key, producer key, count, k, cin, cout, hin, ld)] of the fused pairs' data gradients (cin -> cout channels on the
    hin x hin grid, output rows of ld channels), in backward order of first appearance."""
    tr = YoloTrainer(init_yolo_train_state(scale, nc, seed=0), scale=scale, nc=nc, size=SIZE, batch=BATCH, fused_bn_bwd=True)
    count, first = collections.Counter(), {}
    for pkey, ckey in fused_bn_bwd_pairs(scale, nc).items():
        c = tr.block[ckey]
        sh = (c.k, c.cout, c.cin, tr.geom[ckey][0], tr.act[c.e.src[0]].C)
        count[sh] += 1
        first.setdefault(sh, (ckey, pkey))
    total = sum(1 for b in tr.blocks if b.bn)
    del tr
    torch.cuda.empty_cache()
    return [first[sh] + (n,) + sh for sh, n in count.items()], total


class Pair:
    """Operands of one fused pair: N(0, 1) gradient and pre-activation, N(0, 1 / K) weights (timing does not depend on the values)."""

    def __init__(self, k, cin, cout, hin, ld, g):
        self.args = (BATCH, hin, hin, k, 1)
        self.T, self.C = BATCH * hin * hin, cout
        self.src = yvhip.mview(torch.randn(self.T, cin, generator=g, device=DEV).to(torch.bfloat16))
        self.w = (torch.randn(cout, k * k * cin, generator=g, device=DEV) / math.sqrt(k * k * cin)).to(torch.bfloat16)
        self.da = torch.zeros(self.T, ld, dtype=torch.bfloat16, device=DEV)
        self.z = torch.randn(self.T, cout, generator=g, device=DEV).to(torch.bfloat16)
        self.dz = torch.zeros(self.T, cout, dtype=torch.bfloat16, device=DEV)
        self.ws = torch.zeros(yvhip.bn_ws_floats(self.T, cout), device=DEV)
        self.pw = torch.zeros(yvhip.conv_bnbwd_ws_floats(self.T, cout), device=DEV)
        self.st = [torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV), torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)]
        self.dg, self.db = torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV)
        self.dav, self.zv, self.dzv = yvhip.mview(self.da, ld - cout, cout), yvhip.mview(self.z), yvhip.mview(self.dz)
        self.route = yvhip.conv_bnbwd_route(BATCH, hin, hin, k, 1, cin, cout, out_ld=ld, res_ld=ld, ldz=cout)

    def conv(self):
        yvhip.conv_view(self.src, *self.args, self.w, self.C, self.dav, res=self.dav)

    def bwd(self):
        yvhip.bn_act_bwd(self.dav, self.zv, self.T, *self.st, self.dg, self.db, self.dzv, self.ws)

    def conv_bnbwd(self):
        yvhip.conv_view_bnbwd(self.src, *self.args, self.w, self.C, self.dav, self.zv, *self.st, self.pw, res=self.dav)

    def finish(self):
        yvhip.bn_act_bwd_finish(self.dav, self.zv, self.T, *self.st, self.dg, self.db, self.dzv, self.pw)

    def arm_a(self):
        self.conv(); self.bwd()

    def arm_b(self):
        self.conv_bnbwd(); self.finish()


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3                                         # us per call


def alternate(fns, seconds):
    """Per function (median, lower quartile, upper quartile) of the microseconds per call, the functions alternating inside every round."""
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
    return [(sorted(v)[len(v) // 2], sorted(v)[len(v) // 4], sorted(v)[(3 * len(v)) // 4]) for v in ts], rounds, inner


def table(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    lines = [f"# python tools/bn_bwd_fused_bench.py   ({torch.cuda.get_device_name(0)}; {BATCH} x {SIZE} x {SIZE}; us per sequence, median of "
             f"alternating rounds, >= {MIN_SECONDS} s of launches per arm; A q25..q75: the quartiles of arm A's rounds; route: yv_conv2d_bnbwd_route, "
             f"instance + 16 where the staged epilogue runs)"]
    for scale, nc in MODELS:
        shapes, total = trainer_pairs(scale, nc)
        lines += [f"== YOLOv8{scale} nc {nc}: {sum(sh[2] for sh in shapes)} eligible pairs of {total} BatchNorm blocks",
                  f"{'consumer -> producer (first of the shape)':44s} {'x':>2s} {'k':>1s} {'cin':>4s} {'cout':>4s} {'hin':>4s} {'ld':>4s} {'T':>8s} {'tiles':>6s} "
                  f"{'route':>5s} {'use':>3s} | {'A us':>8s} {'A q25..q75':>15s} {'B us':>8s} {'B - A':>8s} {'B / A':>6s} | {'conv_ws':>8s} {'bn_bwd':>8s} |"
                  f" {'conv_bnbwd':>10s} {'finish':>8s}"]
        print("\n".join(lines[-2:]), flush=True)
        tot = collections.defaultdict(float)
        for ckey, pkey, n, k, cin, cout, hin, ld in shapes:
            p = Pair(k, cin, cout, hin, ld, g)
            ((a, a_lo, a_hi), (b, _, _)), rounds, inner = alternate([p.arm_a, p.arm_b], MIN_SECONDS)
            parts, _, _ = alternate([p.conv, p.bwd, p.conv_bnbwd, p.finish], MIN_SECONDS / 5)
            pc, pb, pcb, pf = (v[0] for v in parts)
            verdict = "level" if a_lo <= b <= a_hi else ("faster" if b < a else "SLOWER")
            lines.append(f"{ckey + ' -> ' + pkey:44s} {n:2d} {k:1d} {cin:4d} {cout:4d} {hin:4d} {ld:4d} {p.T:8d} {p.route.tiles:6d} "
                         f"{p.route.kernel + 16 * p.route.staged:5d} {int(p.route.use):3d} | {a:8.1f} {a_lo:7.1f}..{a_hi:<7.1f} {b:8.1f} {b - a:+8.1f} {b / a:6.3f} |"
                         f" {pc:8.1f} {pb:8.1f} | {pcb:10.1f} {pf:8.1f}  {verdict}")
            print(lines[-1] + f"   ({rounds} rounds of {inner})", flush=True)
            tot["a"] += n * a; tot["b"] += n * b
            tot["used"] += n * (b - a) * p.route.use
            tot["saved"] += n * max(a - b, 0.0); tot["lost"] += n * max(b - a, 0.0)
            tot["epi"] += n * (pcb - pc); tot["fin"] += n * (pb - pf)
            del p
        lines.append(f"  sum over the step's eligible pairs (us): A {tot['a']:.0f}, B {tot['b']:.0f}, B - A {tot['b'] - tot['a']:+.0f}, over the "
                     f"pairs the route fuses {tot['used']:+.0f} (saved "
                     f"{tot['saved']:.0f} on the shapes that win, lost {tot['lost']:.0f} on those that lose); by the parts: the epilogue "
                     f"costs {tot['epi']:+.0f} (conv_bnbwd - conv_ws), the finaliser saves {tot['fin']:+.0f} (bn_bwd - finish)")
        print(lines[-1], flush=True)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    yvhip.require_gpu()
    table(sys.argv[2] if sys.argv[1:2] == ["--out"] else None)
