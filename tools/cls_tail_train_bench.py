#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): the trainer's cls-row tail (VitTrainer(cls_tail=True)).

  python3 tools/cls_tail_train_bench.py          kernels: yv_attention_cls_train + yv_attention_cls_bwd against the pair they replace
                                                 in the last block (yv_attention_train + yv_attention_bwd, or the _long entries above
                                                 224 tokens) at (R, N, H) in (32, 197, 12), (128, 197, 12), (32, 785, 12), with the
                                                 byte floor of the two new kernels: forward K + V once, backward (2 reads + 3 writes)
                                                 x N x 128 B per (crop, head), at 6.3 TB/s
  python3 tools/cls_tail_train_bench.py step     VitTrainer.forward + backward with cls_tail off and on: vit_base_patch16_224 at 32
                                                 and 128 crops, vit_base_patch8_224 at 32 crops (long_attn and long_attn_bwd on in
                                                 both arms), bf16 and mxfp8
  python3 tools/cls_tail_train_bench.py one      three calls of each new kernel at (32, 197, 12) and nothing else: the program for a
                                                 counter or trace run

Each arm is warmed, then the arms take turns in batches timed with device events until each has at least 0.5 s of calls
(CTTB_SECONDS); the figure is the median batch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

yvhip.require_gpu()
dev = "cuda:0"
SECONDS = float(os.environ.get("CTTB_SECONDS", 0.5))
SHAPES = [(32, 197, 12), (128, 197, 12), (32, 785, 12)]
STEPS = [("vit_base_patch16_224", 32), ("vit_base_patch16_224", 128), ("vit_base_patch8_224", 32)]
HBM = 6.3e12


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


def kernel_arms(R, N, H, seed):
    D = H * 64
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    dout = torch.randn(R * N, D, generator=g).to(torch.bfloat16).to(dev)
    dout_c = dout[::N].contiguous()
    z16 = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=dev)
    out, lse, dqkv, delta = z16(R * N, D), torch.zeros(R * H * N, device=dev), z16(R * N, 3 * D), torch.zeros(R * H * N, device=dev)
    out_c, lse_c, dqkv_c = z16(R, D), torch.zeros(R * H, device=dev), z16(R * N, 3 * D)
    q = qkv[::N, :D]
    long_ = N > 224
    fwd = (lambda: yvhip.attention_long(qkv, R, N, H, out, lse=lse)) if long_ else (lambda: yvhip.attention_train(qkv, R, N, H, out, lse))
    bwd = getattr(yvhip, "attention_bwd_long" if long_ else "attention_bwd")
    fwd(); yvhip.attention_cls_train(q, qkv, R, N, H, out_c, lse_c)
    names = ("attention_long" if long_ else "attention_train", "attention_bwd_long" if long_ else "attention_bwd")
    return {names[0]: fwd,
            "attention_cls_train": lambda: yvhip.attention_cls_train(q, qkv, R, N, H, out_c, lse_c),
            names[1]: lambda: bwd(qkv, out, dout, lse, R, N, H, dqkv, delta),
            "attention_cls_bwd": lambda: yvhip.attention_cls_bwd(q, qkv, dout_c, lse_c, R, N, H, dqkv_c)}


def kernels():
    print(f"# the last block's attention: full-row pair and cls pair, alternating; >= {SECONDS} s of calls per arm; floor at 6.3 TB/s")
    for R, N, H in SHAPES:
        arms = kernel_arms(R, N, H, N + H)
        res = alternate(arms)
        floor = {"attention_cls_train": 2.0 * R * H * N * 128 / HBM * 1e6, "attention_cls_bwd": 5.0 * R * H * N * 128 / HBM * 1e6}
        for name, (us, n) in res.items():
            f = f"  floor {floor[name]:6.2f} us ({100.0 * floor[name] / us:4.1f} %)" if name in floor else ""
            print(f"R={R:3d} N={N} H={H:2d} {name:20s} {us:9.1f} us/call  ({n} calls){f}", flush=True)
        k = list(res)
        print(f"R={R:3d} N={N} H={H:2d} full pair {res[k[0]][0] + res[k[2]][0]:8.1f} us, cls pair {res[k[1]][0] + res[k[3]][0]:7.1f} us",
              flush=True)
        del arms
        torch.cuda.empty_cache()


def step():
    from yvhip import engines
    from yvhip.training import VitTrainer
    print(f"# VitTrainer.forward + backward with cls_tail off and on, alternating; >= {SECONDS} s of steps per arm")
    for name, R in STEPS:
        sd = engines.init_vit_wrapper_state(name, 5, seed=4)
        g = torch.Generator().manual_seed(R)
        labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).to(dev)
        for dtype in ("bf16", "mxfp8"):
            long_ = engines.vit_cfg(name)[0] == 8
            tr = {flag: VitTrainer(sd, name, 5, device=dev, dtype=dtype, long_attn=long_, long_attn_bwd=long_, cls_tail=flag)
                  for flag in (False, True)}
            t0 = tr[False]
            pm = (torch.rand(R * t0.tok, 3 * t0.P_ * t0.P_, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)

            def arm(flag):
                def run():
                    tr[flag].forward(pm, R)
                    tr[flag].backward(pm, labels, R)
                return run
            res = alternate({"cls_tail=False": arm(False), "cls_tail=True": arm(True)})
            for k, (us, n) in res.items():
                print(f"{name} {dtype:5s} {R:3d} crops {k:14s} {us * 1e-3:8.3f} ms/step  {R / us * 1e6:8.1f} crops/s  ({n} steps)",
                      flush=True)
            off, on = res["cls_tail=False"][0], res["cls_tail=True"][0]
            print(f"{name} {dtype:5s} {R:3d} crops off / on time {off / on:.3f} x ({(off - on) * 1e-3:+.3f} ms)", flush=True)
            del tr, t0
            torch.cuda.empty_cache()


def one():
    arms = kernel_arms(*SHAPES[0], 1)
    for _ in range(3):
        arms["attention_cls_train"]()
        arms["attention_cls_bwd"]()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"step": step, "one": one}.get(" ".join(sys.argv[1:]), kernels)()
