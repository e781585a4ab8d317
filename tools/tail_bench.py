#!/usr/bin/env python3
"""Dev tool (GPU box): the cls-row tail of the classifier's last block, kernel by kernel.  The five tail products (q, proj, fc1,
fc2, head of ViT-B/16) at 64 and 128 rows on the old route (128 x 128 tiles: yv_set_option("linear_skinny", 0)) and on the
skinny route, interleaved in one process, and yv_attention_cls at 64 / 128 crops; each as us and as a share of its bound
(weights read once / K + V bytes read once, over 6.3 TB/s achievable HBM rate).  Every launch of a timed chain uses another
copy of its weights / its qkv buffer (TB_COPIES, default 12: ~57 MB of fc2 weights, more than the L2s hold), as in the
pipeline, where a whole step lies between two uses.  The products are timed by events attached to the launch itself
(yv_set_launch_timing: the kernel alone - a back-to-back chain of 10 us kernels measures the host's enqueue rate instead); the
attention figures are chain times (an upper bound: profiles/cls_tail_kernel_stats_after.csv has the kernel alone)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

dev = "cuda:0"
HBM = 6.3e12
COPIES = int(os.environ.get("TB_COPIES", 12))
D, N, H = 768, 197, 12
E = yvhip
shapes = [("q", D, D, 0, torch.bfloat16, False), ("proj", D, D, E.EPI_RES_F32, torch.float32, True),
          ("fc1", 4 * D, D, E.EPI_GELU, torch.bfloat16, False), ("fc2", D, 4 * D, E.EPI_RES_F32, torch.float32, True),
          ("head", 1024, D, E.EPI_OUT_F32, torch.float32, False)]
g = torch.Generator().manual_seed(0)


def timed(fn, n):
    fn(0); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per launch


def timed_linear(fn, n):
    """Median kernel time (us) of n launches, from the start / stop timestamps of each launch's own dispatch packet."""
    recs = []
    fn(0); torch.cuda.synchronize()
    yvhip.reserve_events(2 * n)
    yvhip.LINEAR_HOOK = lambda M, N, K, e0, e1: recs.append((e0, e1))
    try:
        for i in range(n):
            fn(i)
    finally:
        yvhip.LINEAR_HOOK = None
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in recs)
    return ts[len(ts) // 2]


for rows in (64, 128):
    cnt = torch.tensor([rows], dtype=torch.int32, device=dev)
    total = {0: 0.0, 256: 0.0}
    for name, n, k, flags, odt, strided in shapes:
        a = torch.randn(rows, k, generator=g).to(torch.bfloat16).to(dev)
        ws = [(torch.randn(n, k, generator=g) * 0.05).to(torch.bfloat16).to(dev) for _ in range(COPIES)]
        bias = torch.randn(n, generator=g).to(dev)
        # the residual products write the cls rows of the token stream (row stride N * D), the others a compact buffer
        full = torch.zeros(rows * (N if strided else 1), n, dtype=odt, device=dev)
        out = full[::N] if strided else full
        res = {0: [], 256: []}
        for rd in range(5):
            for bound in (0, 256):
                yvhip.set_option("linear_skinny", bound)
                res[bound].append(timed_linear(lambda i: yvhip.linear(a, ws[i % COPIES], bias, out, flags=flags, m_dev=cnt, m_mul=1),
                                        2 * COPIES))
        yvhip.set_option("linear_skinny", 256)
        floor = n * k * 2 / HBM * 1e6
        old, new = sorted(res[0])[2], sorted(res[256])[2]
        total[0] += old; total[256] += new
        print(f"{name:5s} M={rows:3d} N={n:4d} K={k:4d}: tiled {old:6.1f} us  skinny {new:6.1f} us  "
              f"weights-once floor {floor:5.2f} us ({floor / new * 100:4.1f} % of the skinny time)", flush=True)
    print(f"five products at {rows} rows: tiled {total[0]:.1f} us, skinny {total[256]:.1f} us (kernels alone)")
    qkvs = [(torch.randn(rows * N, 3 * D, generator=g)).to(torch.bfloat16).to(dev) for _ in range(4)]
    q = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
    o = torch.zeros(rows, D, dtype=torch.bfloat16, device=dev)
    of = torch.zeros(rows * N, D, dtype=torch.bfloat16, device=dev)
    ts = sorted(timed(lambda i: yvhip.attention_cls(q, qkvs[i % 4], rows, N, H, o, r_dev=cnt), 16) for _ in range(5))
    tf = sorted(timed(lambda i: yvhip.attention(qkvs[i % 4], rows, N, H, of, r_dev=cnt), 16) for _ in range(5))
    floor = rows * N * 2 * D * 2 / HBM * 1e6
    print(f"attention_cls {rows:3d} crops: {ts[2]:6.1f} us  K + V once floor {floor:5.2f} us ({floor / ts[2] * 100:4.1f} %)   "
          f"(full attention: {tf[2]:6.1f} us)", flush=True)
