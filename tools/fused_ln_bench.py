#!/usr/bin/env python3
"""Dev tool (GPU box): the residual products of a ViT block with the LayerNorm that follows them, unfused against fused.  Per
shape, the pair yv_linear (YV_EPI_RES_F32) + yv_layernorm and the single yv_linear_res_ln launch, alternated in one process
after a warm-up until each side has been timed for at least FLN_SECONDS (default 0.5) of device time; device events around
chains of FLN_CHAIN launches (default 20).  Successive launches rotate over FLN_COPIES (default 3) sets of activation / stream
/ output buffers, as in the pipeline, where a whole block lies between two uses of a buffer.  Printed per point: us per
launch of each side (median over the chains, min), their ratio, and the fused kernel's share of the MFMA roof
(2 M N K flops over the bf16 dense peak) and of the HBM floor (a read once, x read + written, h written, at 6.3 TB/s)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

dev = "cuda:0"
PEAK, HBM = 2500e12, 6.3e12
SECONDS = float(os.environ.get("FLN_SECONDS", 0.5))
CHAIN = int(os.environ.get("FLN_CHAIN", 20))
COPIES = int(os.environ.get("FLN_COPIES", 3))
g = torch.Generator().manual_seed(0)
print(f"{'M':>6} {'N':>5} {'K':>5} | {'linear+ln us':>13} {'(min)':>8} | {'res_ln us':>10} {'(min)':>8} | {'fused/pair':>10} | "
      f"{'MFMA roof':>9} {'HBM floor':>9}")
for N, K in ((768, 768), (768, 3072), (1024, 1024), (1024, 4096)):
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    bias, gamma, beta = torch.randn(N, generator=g).to(dev), (1 + 0.1 * torch.randn(N, generator=g)).to(dev), torch.randn(N, generator=g).to(dev)
    for M in (6304, 12608, 25216):
        a = [torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev) for _ in range(COPIES)]
        x = [torch.zeros(M, N, device=dev) for _ in range(COPIES)]
        h = [torch.zeros(M, N, dtype=torch.bfloat16, device=dev) for _ in range(COPIES)]

        def pair(i):
            c = i % COPIES
            yvhip.linear(a[c], w, bias, x[c], flags=yvhip.EPI_RES_F32)
            yvhip.layernorm(x[c], gamma, beta, h[c], M, N, N, N)

        def fused(i):
            c = i % COPIES
            yvhip.linear_res_ln(a[c], w, bias, x[c], gamma, beta, h[c])

        def chain(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(CHAIN):
                fn(i)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / CHAIN          # us per launch (pair: per two launches)

        for fn in (pair, fused):
            chain(fn)
        ts = {pair: [], fused: []}
        while min(sum(v) for v in ts.values()) * CHAIN < SECONDS * 1e6:
            for fn in (pair, fused):
                ts[fn].append(chain(fn))
        med = {fn: sorted(v)[len(v) // 2] for fn, v in ts.items()}
        roof = 2.0 * M * N * K / PEAK * 1e6
        floor = (M * K * 2 + M * N * (8 + 2) + N * K * 2) / HBM * 1e6
        print(f"{M:>6} {N:>5} {K:>5} | {med[pair]:>13.1f} {min(ts[pair]):>8.1f} | {med[fused]:>10.1f} {min(ts[fused]):>8.1f} | "
              f"{med[fused] / med[pair]:>10.3f} | {roof / med[fused]:>9.3f} {floor / med[fused]:>9.3f}", flush=True)
        del a, x, h
