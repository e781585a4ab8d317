#!/usr/bin/env python3
"""Dev tool (GPU only; it fails without a device): yv_attention_fp8 against the two kernels an mxfp8 engine
calls today, the qkv product that feeds each, and a VitEngine pass with fp8_attn off and on.  Method of tools/attn_long_bench.py
(its `alternate`): each arm is warmed, then the arms take turns in batches of launches timed with device events until each has at
least 0.5 s of launches (ALB_SECONDS); the figure is the median batch.

  python3 tools/attn_fp8_bench.py            kernels, then the qkv linears, at (R, N, H) in (32, 785, 12), (128, 785, 12),
                                              (64, 577, 12), (128, 197, 12), (256, 197, 16)
  python3 tools/attn_fp8_bench.py kernels [RxNxH ...] | linears [RxNxH ...]
  python3 tools/attn_fp8_bench.py e2e        VitEngine(dtype="mxfp8").backbone + head, 32 and 128 crops, vit_base_patch8_224 (also
                                              with long_attn, the faster unflagged form there), vit_base_patch16_224 and
                                              vit_large_patch16_224, fp8_attn off and on

kernels: every arm writes the proj operand (out_q / out_scale).  attention_long and attention_mxfp8 read the bf16 qkv, attention_fp8
its yv_quant_mxfp8 image; bytes = the qkv read once plus the MX output written once.  linears: the qkv product (rows R N, K = 64 H,
3 K columns) as linear_mxfp8 (bf16 output) and as linear_mxfp8_q (MXFP8 output, flags = 0)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import yvhip
from attn_long_bench import SECONDS, alternate, dev

SHAPES = [(32, 785, 12), (128, 785, 12), (64, 577, 12), (128, 197, 12), (256, 197, 16)]


def r256(n):
    return (n + 255) // 256 * 256


def kernels(shapes):
    print(f"# attention writing the proj operand: attention_long / attention_mxfp8 (bf16 qkv) and attention_fp8 (MXFP8 qkv), "
          f"alternating; >= {SECONDS} s of launches per arm")
    for R, N, H in shapes:
        D, rows = H * 64, R * N
        g = torch.Generator().manual_seed(N + H)
        qkv = (torch.randn(rows, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        q8, s8 = yvhip.quant_mxfp8(qkv)
        names = ("attention_long", "attention_mxfp8", "attention_fp8")
        oq = {k: torch.zeros(rows, D, dtype=torch.uint8, device=dev) for k in names}
        os_ = {k: torch.zeros(D // 128, r256(rows), 4, dtype=torch.uint8, device=dev) for k in names}
        arms = {"attention_long": lambda: yvhip.attention_long(qkv, R, N, H, out_q=oq["attention_long"], out_scale=os_["attention_long"]),
                "attention_mxfp8": lambda: yvhip.attention_mxfp8(qkv, R, N, H, oq["attention_mxfp8"], os_["attention_mxfp8"]),
                "attention_fp8": lambda: yvhip.attention_fp8(q8, s8, R, N, H, out_q=oq["attention_fp8"], out_scale=os_["attention_fp8"])}
        res = alternate(arms)
        flop = 4.0 * R * H * N * N * 64
        byts = {"attention_long": rows * (6 * D + D * 33 / 32), "attention_mxfp8": rows * (6 * D + D * 33 / 32),
                "attention_fp8": rows * (3 * D * 33 / 32 + D * 33 / 32)}
        for name, (us, n) in res.items():
            print(f"R={R:3d} N={N} H={H:2d} {name:15s} {us:9.1f} us/launch  {flop / us * 1e-6:7.1f} useful TFLOP/s  "
                  f"{byts[name] / us * 1e-3:7.1f} useful GB/s  ({n} launches)", flush=True)
        same = float((oq["attention_fp8"] == oq["attention_long"]).float().mean())
        fp8 = res["attention_fp8"][0]
        print(f"R={R:3d} N={N} H={H:2d} attention_long / attention_fp8 time {res['attention_long'][0] / fp8:.3f} x, attention_mxfp8 / "
              f"attention_fp8 {res['attention_mxfp8'][0] / fp8:.3f} x; output bytes equal to attention_long's: {same:.3f}", flush=True)


def linears(shapes):
    print(f"# the qkv product: linear_mxfp8 (bf16 output) and linear_mxfp8_q (MXFP8 output), alternating; >= {SECONDS} s per arm")
    for R, N, H in shapes:
        D, rows = H * 64, R * N
        g = torch.Generator().manual_seed(N + H + 1)
        a = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
        w = (torch.randn(3 * D, D, generator=g) * 0.04).to(torch.bfloat16).to(dev)
        bias = (torch.randn(3 * D, generator=g) * 0.02).to(dev)
        aq, asc = yvhip.quant_mxfp8(a)
        wq, wsc = yvhip.quant_mxfp8(w)
        out = torch.zeros(rows, 3 * D, dtype=torch.bfloat16, device=dev)
        q = torch.zeros(rows, 3 * D, dtype=torch.uint8, device=dev)
        s = torch.zeros(3 * D // 128, r256(rows), 4, dtype=torch.uint8, device=dev)
        res = alternate({"linear_mxfp8": lambda: yvhip.linear_mxfp8(aq, asc, wq, wsc, bias, out),
                         "linear_mxfp8_q": lambda: yvhip.linear_mxfp8_q(aq, asc, wq, wsc, bias, q, s)})
        flop = 2.0 * rows * D * 3 * D
        for name, (us, n) in res.items():
            print(f"rows={rows:6d} K={D:4d} N={3 * D:4d} {name:15s} {us:9.1f} us/launch  {flop / us * 1e-6:7.1f} TFLOP/s  ({n} launches)",
                  flush=True)
        print(f"rows={rows:6d} K={D:4d} N={3 * D:4d} linear_mxfp8 / linear_mxfp8_q time "
              f"{res['linear_mxfp8'][0] / res['linear_mxfp8_q'][0]:.3f} x", flush=True)


def e2e():
    from yvhip import engines
    print(f"# VitEngine(dtype='mxfp8').backbone + head, fp8_attn off and on, alternating; >= {SECONDS} s of passes per arm")
    for name in ("vit_base_patch8_224", "vit_base_patch16_224", "vit_large_patch16_224"):
        sd = engines.init_vit_wrapper_state(name, 5, seed=4)
        kws = {"off": dict(), "on": dict(fp8_attn=True)}
        if "patch8" in name:
            kws["off, long_attn"] = dict(long_attn=True)
        eng = {k: engines.VitEngine(sd, name, 5, device=dev, dtype="mxfp8", **kw) for k, kw in kws.items()}
        del sd
        for R in (32, 128):
            cnt = torch.tensor([R], dtype=torch.int32, device=dev)
            logits = torch.zeros(R, 5, device=dev)
            labels = torch.zeros(R, dtype=torch.int32, device=dev)
            feats = {}

            def arm(k):
                e = eng[k]
                buf = e.patch_buffer(R)
                buf.copy_((torch.rand(buf.shape, generator=torch.Generator().manual_seed(R)) * 2 - 1).to(torch.bfloat16))

                def run():
                    with e.guard():
                        feats[k] = e.backbone(buf, R, cnt)
                        e.head(feats[k], R, logits, labels, count=cnt)
                return run
            res = alternate({k: arm(k) for k in eng})
            b = feats["off"][:, :1000].double()
            for k, (us, n) in res.items():
                print(f"{name} {R:3d} crops fp8_attn {k:14s} {us * 1e-3:8.2f} ms/pass  {R / us * 1e6:8.1f} crops/s  ({n} passes)", flush=True)
            best_off = min(us for k, (us, _) in res.items() if k != "on")
            print(f"{name} {R:3d} crops off / on time {res['off'][0] / res['on'][0]:.3f} x (best unflagged / on {best_off / res['on'][0]:.3f} x), "
                  f"backbone logits rel-L2 on vs off {float((feats['on'][:, :1000].double() - b).norm() / b.norm()):.2e}", flush=True)
            for e in eng.values():
                e._bufs.clear()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    mode, rest = (sys.argv[1:2] or ["all"])[0], sys.argv[2:]
    shapes = [tuple(int(v) for v in a.split("x")) for a in rest] or SHAPES
    if mode == "e2e":
        e2e()
    elif mode == "kernels":
        kernels(shapes)
    elif mode == "linears":
        linears(shapes)
    else:
        kernels(SHAPES)
        linears(SHAPES)
