#!/usr/bin/env python3
"""Dev tool (GPU box): four isolated launches of yv_linear_res_ln and of the unfused yv_linear (f32 residual) at ViT-B's fc2 shape,
for counter runs: rocprofv3 --pmc <counters> --output-format csv -d DIR -- python3 tools/fused_ln_one.py, then
tools/pmc_kernel_summary.py DIR gemm_res_ln (or gemm_p9)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch, yvhip
dev = "cuda:0"
M, N, K = 12608, 768, 3072
g = torch.Generator().manual_seed(0)
a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).to(dev)
bias, gamma, beta = torch.randn(N).to(dev), torch.ones(N).to(dev), torch.zeros(N).to(dev)
x = torch.zeros(M, N, device=dev); h = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
for i in range(4):
    yvhip.linear_res_ln(a, w, bias, x, gamma, beta, h)
    yvhip.linear(a, w, bias, x, flags=yvhip.EPI_RES_F32)
    torch.cuda.synchronize()
