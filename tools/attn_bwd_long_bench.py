#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): yv_attention_bwd against yv_attention_bwd_long at the sequence lengths that
do not fit one tile, alternating in one process.

  python3 tools/attn_bwd_long_bench.py          kernels: (R, N, H) in (32, 785, 12), (128, 785, 12), (64, 577, 12), (64, 577, 16);
                                                a call is both kernels (dQ + delta, dK / dV) of its entry point
  python3 tools/attn_bwd_long_bench.py step     the vit_base_patch8_224 trainer step (VitTrainer.forward + backward, ABLB_CROPS =
                                                32 crops, bf16 and mxfp8) with long_attn_bwd off and on, and the share of the
                                                step that is attention backward (L calls at the step's shape, timed alone)
  python3 tools/attn_bwd_long_bench.py one      three calls of each entry point at (32, 785, 12) and nothing else: the program
                                                for a counter run (rocprofv3 --pmc ... -- python3 tools/attn_bwd_long_bench.py one)

Each arm is warmed, then the arms take turns in batches of launches timed with device events until each has at least 0.5 s of
launches (ABLB_SECONDS); the figure is the median batch.  Per arm: us per call and useful TFLOP/s (7 products: 14 R H N^2 64 over
the time); per shape whether the two arms' dqkv and delta are the same bits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

yvhip.require_gpu()
dev = "cuda:0"
SECONDS = float(os.environ.get("ABLB_SECONDS", 0.5))
CROPS = int(os.environ.get("ABLB_CROPS", 32))
SHAPES = [(32, 785, 12), (128, 785, 12), (64, 577, 12), (64, 577, 16)]
ARMS = ("attention_bwd", "attention_bwd_long")


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
    """-> ({arm: fn}, {arm: (dqkv, delta)}) on random operands with the forward's own out and lse"""
    D = H * 64
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    dout = torch.randn(R * N, D, generator=g).to(torch.bfloat16).to(dev)
    out = torch.zeros(R * N, D, dtype=torch.bfloat16, device=dev)
    lse = torch.zeros(R * H * N, device=dev)
    yvhip.attention_train(qkv, R, N, H, out, lse)
    res = {k: (torch.zeros(R * N, 3 * D, dtype=torch.bfloat16, device=dev), torch.zeros(R * H * N, device=dev)) for k in ARMS}
    arms = {k: (lambda k=k: getattr(yvhip, k)(qkv, out, dout, lse, R, N, H, *res[k])) for k in ARMS}
    return arms, res


def kernels():
    print(f"# yv_attention_bwd (parent kernels) and yv_attention_bwd_long, alternating; >= {SECONDS} s of calls per arm")
    for R, N, H in SHAPES:
        arms, out = bwd_arms(R, N, H, N + H)
        res = alternate(arms)
        flop = 14.0 * R * H * N * N * 64
        for name, (us, n) in res.items():
            print(f"R={R:3d} N={N} H={H:2d} {name:18s} {us:9.1f} us/call  {flop / us * 1e-6:7.1f} useful TFLOP/s  ({n} calls)",
                  flush=True)
        same = all(torch.equal(a, b) for a, b in zip(out[ARMS[0]], out[ARMS[1]]))
        print(f"R={R:3d} N={N} H={H:2d} attention_bwd / attention_bwd_long time {res[ARMS[0]][0] / res[ARMS[1]][0]:.2f} x, "
              f"dqkv and delta bit-identical: {same}", flush=True)
        del arms, out
        torch.cuda.empty_cache()


def step():
    from yvhip import engines
    from yvhip.training import VitTrainer
    name, R = "vit_base_patch8_224", CROPS
    print(f"# {name}: VitTrainer.forward + backward, {R} crops, long_attn_bwd off and on, alternating; >= {SECONDS} s of steps "
          f"per arm; attention backward alone: L calls at (R, N, H) of the step, alternating")
    sd = engines.init_vit_wrapper_state(name, 5, seed=4)
    g = torch.Generator().manual_seed(R)
    labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(dev)
    for dtype in ("bf16", "mxfp8"):
        tr = {flag: VitTrainer(sd, name, 5, device=dev, dtype=dtype, long_attn_bwd=flag) for flag in (False, True)}
        t0 = tr[False]
        pm = (torch.rand(R * t0.tok, 3 * t0.P_ * t0.P_, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)

        def arm(flag):
            def run():
                tr[flag].forward(pm, R)
                tr[flag].backward(pm, labels, R)
            return run
        res = alternate({"long_attn_bwd=False": arm(False), "long_attn_bwd=True": arm(True)})
        ga, gb = tr[False].grad_dict(), tr[True].grad_dict()
        same = all(torch.equal(ga[k], gb[k]) for k in ga)
        arms, _ = bwd_arms(R, t0.N, t0.H, R)
        alone = alternate(arms)
        for (k, (us, n)), a in zip(res.items(), ARMS):
            bwd_us = alone[a][0] * t0.L
            print(f"{dtype:5s} {R:3d} crops {k:19s} {us * 1e-3:8.2f} ms/step  {R / us * 1e6:8.1f} crops/s  ({n} steps); "
                  f"{t0.L} x {a} alone {bwd_us * 1e-3:7.2f} ms = {100.0 * bwd_us / us:4.1f} % of the step", flush=True)
        print(f"{dtype:5s} {R:3d} crops off / on time {res['long_attn_bwd=False'][0] / res['long_attn_bwd=True'][0]:.3f} x, "
              f"gradients bit-identical: {same}", flush=True)
        del tr, t0, arms
        torch.cuda.empty_cache()


def one():
    arms, _ = bwd_arms(*SHAPES[0], 1)
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"step": step, "one": one}.get(" ".join(sys.argv[1:]), kernels)()
