#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): yv_attention_bwd, yv_attention_bwd_long and the one-launch
yv_attention_bwd_short at 197 tokens, alternating in one process.

  python3 tools/attn_bwd_short_bench.py         kernels: (R, N, H) in (32, 197, 12), (64, 197, 12), (128, 197, 12), (64, 197, 16);
                                                a call is every kernel of its entry point (two, two, one)
  python3 tools/attn_bwd_short_bench.py step    the vit_base_patch16_224 trainer step (VitTrainer.forward + backward, bf16 and
                                                mxfp8, 32 and 128 crops: ABSB_CROPS) with short_attn_bwd off and on, and the share
                                                of the step that is attention backward (L calls at the step's shape, timed alone)
  python3 tools/attn_bwd_short_bench.py one     three calls of each entry point at (32, 197, 12) and nothing else: the program
                                                for a trace or counter run (rocprofv3 ... -- python3 tools/attn_bwd_short_bench.py one)

The arms' dqkv and delta are compared bit for bit BEFORE anything is timed; a difference ends the run.  Each arm is warmed, then
the arms take turns in batches of launches timed with device events until each has at least 0.5 s of launches (ABSB_SECONDS);
the figure is the median batch.  Per arm: us per call and useful TFLOP/s (7 products: 14 R H N^2 64 over the time)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

yvhip.require_gpu()
dev = "cuda:0"
SECONDS = float(os.environ.get("ABSB_SECONDS", 0.5))
CROPS = [int(c) for c in os.environ.get("ABSB_CROPS", "32,128").split(",")]
SHAPES = [(32, 197, 12), (64, 197, 12), (128, 197, 12), (64, 197, 16)]
ARMS = ("attention_bwd", "attention_bwd_long", "attention_bwd_short")


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms):
    """arms: {name: fn}.  -> {name: (median us per call, calls timed)}"""
    per = {}
    for name, fn in arms.items():                       # warm, and size the batches to ~50 ms
        batch_ms(fn, 3)
        per[name] = max(1, int(50.0 / max(batch_ms(fn, 3) / 3, 1e-3)))
    got = {name: [] for name in arms}
    while any(sum(v) < SECONDS * 1e3 for v in got.values()):
        for name, fn in arms.items():
            got[name].append(batch_ms(fn, per[name]))
    return {name: (sorted(v)[len(v) // 2] / per[name] * 1e3, len(v) * per[name]) for name, v in got.items()}


def bwd_arms(R, N, H, seed):
    """-> {arm: fn} on random operands with the forward's own out and lse; the arms' results are verified to be the same bits"""
    D = H * 64
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    dout = torch.randn(R * N, D, generator=g).to(torch.bfloat16).to(dev)
    out = torch.zeros(R * N, D, dtype=torch.bfloat16, device=dev)
    lse = torch.zeros(R * H * N, device=dev)
    yvhip.attention_train(qkv, R, N, H, out, lse)
    res = {k: (torch.zeros(R * N, 3 * D, dtype=torch.bfloat16, device=dev), torch.zeros(R * H * N, device=dev)) for k in ARMS}
    arms = {k: (lambda k=k: getattr(yvhip, k)(qkv, out, dout, lse, R, N, H, *res[k])) for k in ARMS}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for k in ARMS[1:]:
        if not all(torch.equal(a, b) and bool(torch.isfinite(a.float()).all()) for a, b in zip(res[ARMS[0]], res[k])):
            raise SystemExit(f"R={R} N={N} H={H}: {k} and {ARMS[0]} differ in dqkv or delta")
    return arms


def kernels():
    print(f"# yv_attention_bwd (two kernels), yv_attention_bwd_long (two kernels) and yv_attention_bwd_short (one launch), "
          f"alternating; >= {SECONDS} s of calls per arm; dqkv and delta verified bit-identical before timing")
    for R, N, H in SHAPES:
        arms = bwd_arms(R, N, H, N + H)
        print(f"R={R:3d} N={N} H={H:2d} dqkv and delta of the three arms bit-identical: True", flush=True)
        res = alternate(arms)
        flop = 14.0 * R * H * N * N * 64
        for name, (us, n) in res.items():
            print(f"R={R:3d} N={N} H={H:2d} {name:19s} {us:9.1f} us/call  {flop / us * 1e-6:7.1f} useful TFLOP/s  ({n} calls)",
                  flush=True)
        base = res[ARMS[0]][0]
        print(f"R={R:3d} N={N} H={H:2d} time of attention_bwd over attention_bwd_long {base / res[ARMS[1]][0]:.2f} x, "
              f"over attention_bwd_short {base / res[ARMS[2]][0]:.2f} x", flush=True)
        del arms
        torch.cuda.empty_cache()


def step():
    from yvhip import engines
    from yvhip.training import VitTrainer
    name = "vit_base_patch16_224"
    print(f"# {name}: VitTrainer.forward + backward, short_attn_bwd off and on, alternating; >= {SECONDS} s of steps per arm; "
          f"attention backward alone: L calls at (R, N, H) of the step, alternating")
    sd = engines.init_vit_wrapper_state(name, 5, seed=4)
    for dtype in ("bf16", "mxfp8"):
        for R in CROPS:
            g = torch.Generator().manual_seed(R)
            labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(dev)
            tr = {flag: VitTrainer(sd, name, 5, device=dev, dtype=dtype, short_attn_bwd=flag) for flag in (False, True)}
            t0 = tr[False]
            pm = (torch.rand(R * t0.tok, 3 * t0.P_ * t0.P_, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)

            def arm(flag):
                def run():
                    tr[flag].forward(pm, R)
                    tr[flag].backward(pm, labels, R)
                return run
            for flag in (False, True):
                arm(flag)()
            torch.cuda.synchronize()
            ga, gb = tr[False].grad_dict(), tr[True].grad_dict()
            if not all(torch.equal(ga[k], gb[k]) for k in ga):
                raise SystemExit(f"{dtype} {R} crops: the gradients of short_attn_bwd off and on differ")
            res = alternate({"short_attn_bwd=False": arm(False), "short_attn_bwd=True": arm(True)})
            alone = alternate(bwd_arms(R, t0.N, t0.H, R))
            for (k, (us, n)), a in zip(res.items(), (ARMS[0], ARMS[2])):
                bwd_us = alone[a][0] * t0.L
                print(f"{dtype:5s} {R:3d} crops {k:20s} {us * 1e-3:8.2f} ms/step  {R / us * 1e6:8.1f} crops/s  ({n} steps); "
                      f"{t0.L} x {a} alone {bwd_us * 1e-3:7.2f} ms = {100.0 * bwd_us / us:4.1f} % of the step", flush=True)
            print(f"{dtype:5s} {R:3d} crops off / on time {res['short_attn_bwd=False'][0] / res['short_attn_bwd=True'][0]:.3f} x, "
                  f"gradients bit-identical: True", flush=True)
            del tr, t0
            torch.cuda.empty_cache()


def one():
    arms = bwd_arms(*SHAPES[0], 1)
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"step": step, "one": one}.get(" ".join(sys.argv[1:]), kernels)()
