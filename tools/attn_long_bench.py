#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): yv_attention against yv_attention_long at the sequence lengths that do not fit
one K/V tile, alternating in one process.

  python3 tools/attn_long_bench.py            kernels: (R, N, H) in (32, 785, 12), (128, 785, 12), (64, 577, 12), (64, 577, 16)
  python3 tools/attn_long_bench.py kernels RxNxH ...   the same on the shapes given, e.g. 64x197x12 (both entry points take any N)
  python3 tools/attn_long_bench.py e2e       the classifier alone (VitEngine.backbone + head, vit_base_patch8_224, 32 and 128
                                              crops, bf16 and mxfp8) with long_attn off and on

Each arm is warmed, then the arms take turns in batches of launches timed with device events until each has at least 0.5 s of
launches (ALB_SECONDS); the figure is the median batch.  Per arm: us per launch, useful TFLOP/s (4 R H N^2 64 over the time),
useful bytes/s (qkv read once plus out written once), and the rel-L2 of one sampled crop against fp32 torch; per shape the
maximum |difference| between the two arms' outputs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

yvhip.require_gpu()
dev = "cuda:0"
SECONDS = float(os.environ.get("ALB_SECONDS", 0.5))
SHAPES = [(32, 785, 12), (128, 785, 12), (64, 577, 12), (64, 577, 16)]


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms):
    """arms: {name: fn}.  -> {name: (median us per launch, launches timed)}"""
    per = {}
    for name, fn in arms.items():                       # warm, and size the batches to ~50 ms
        batch_ms(fn, 3)
        per[name] = max(1, int(50.0 / max(batch_ms(fn, 3) / 3, 1e-3)))
    got = {name: [] for name in arms}
    while any(sum(v) < SECONDS * 1e3 for v in got.values()):
        for name, fn in arms.items():
            got[name].append(batch_ms(fn, per[name]))
    return {name: (sorted(v)[len(v) // 2] / per[name] * 1e3, len(v) * per[name]) for name, v in got.items()}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def kernels(shapes=SHAPES):
    print(f"# yv_attention (parent kernel) and yv_attention_long, alternating; >= {SECONDS} s of launches per arm")
    for R, N, H in shapes:
        D = H * 64
        g = torch.Generator().manual_seed(N + H)
        qkv = (torch.randn(R * N, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        outs = {k: torch.zeros(R * N, D, dtype=torch.bfloat16, device=dev) for k in ("attention", "attention_long")}
        arms = {"attention": lambda: yvhip.attention(qkv, R, N, H, outs["attention"]),
                "attention_long": lambda: yvhip.attention_long(qkv, R, N, H, outs["attention_long"])}
        res = alternate(arms)
        torch.cuda.synchronize()
        r = R // 2                                      # the sampled crop
        t = qkv[r * N:(r + 1) * N].cpu().float().view(1, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        ref = (((t[0] * 0.125) @ t[1].transpose(-2, -1)).softmax(-1) @ t[2]).transpose(1, 2).reshape(N, D)
        flop, byts = 4.0 * R * H * N * N * 64, R * N * (3 * D + D) * 2.0
        for name, (us, n) in res.items():
            err = rel_l2(outs[name][r * N:(r + 1) * N].cpu().float(), ref)
            print(f"R={R:3d} N={N} H={H:2d} {name:15s} {us:9.1f} us/launch  {flop / us * 1e-6:7.1f} useful TFLOP/s  "
                  f"{byts / us * 1e-3:7.1f} useful GB/s  rel-L2 vs fp32 (crop {r}) {err:.2e}  ({n} launches)", flush=True)
        diff = float((outs["attention"].float() - outs["attention_long"].float()).abs().max())
        print(f"R={R:3d} N={N} H={H:2d} attention / attention_long time {res['attention'][0] / res['attention_long'][0]:.2f} x, "
              f"max |difference| of the outputs {diff:.3e}", flush=True)


def e2e():
    from yvhip import engines
    name = "vit_base_patch8_224"
    print(f"# {name}: VitEngine.backbone + head, long_attn off and on, alternating; >= {SECONDS} s of passes per arm")
    sd = engines.init_vit_wrapper_state(name, 5, seed=4)
    for dtype in ("bf16", "mxfp8"):
        eng = {flag: engines.VitEngine(sd, name, 5, device=dev, dtype=dtype, long_attn=flag) for flag in (False, True)}
        for R in (32, 128):
            g = torch.Generator().manual_seed(R)
            cnt = torch.tensor([R], dtype=torch.int32, device=dev)
            logits = torch.zeros(R, 5, device=dev)
            labels = torch.zeros(R, dtype=torch.int32, device=dev)
            feats = {}

            def arm(flag):
                e = eng[flag]
                buf = e.patch_buffer(R)
                buf.copy_((torch.rand(buf.shape, generator=g) * 2 - 1).to(torch.bfloat16))

                def run():
                    with e.guard():
                        feats[flag] = e.backbone(buf, R, cnt)
                        e.head(feats[flag], R, logits, labels, count=cnt)
                return run
            g.manual_seed(R)
            off = arm(False)
            g.manual_seed(R)
            on = arm(True)
            res = alternate({"long_attn=False": off, "long_attn=True": on})
            a, b = feats[True][:, :1000].double(), feats[False][:, :1000].double()
            for k, (us, n) in res.items():
                print(f"{dtype:5s} {R:3d} crops {k:15s} {us * 1e-3:8.2f} ms/pass  {R / us * 1e6:8.1f} crops/s  ({n} passes)", flush=True)
            print(f"{dtype:5s} {R:3d} crops off / on time {res['long_attn=False'][0] / res['long_attn=True'][0]:.3f} x, "
                  f"backbone logits rel-L2 on vs off {float((a - b).norm() / b.norm()):.2e}", flush=True)
            for e in eng.values():
                e._bufs.clear()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if sys.argv[1:] == ["e2e"]:
        e2e()
    elif sys.argv[1:2] == ["kernels"] and sys.argv[2:]:
        kernels([tuple(int(v) for v in a.split("x")) for a in sys.argv[2:]])
    else:
        kernels()
