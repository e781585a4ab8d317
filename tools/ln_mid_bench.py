#!/usr/bin/env python3
"""Dev tool (GPU box): norm1 -> qkv and norm2 -> fc1 of ViT-B/16, ViT-B/8 and ViT-L/16 at 1 .. 16 crops - the classifier as
DetectClassifyPipeline(fit_crops=True) sizes it - on two arms, interleaved in one process:
  pair   layernorm + linear as VitEngine(mid_gemm=True) routes it ("linear_mid" = MID_GEMM_ROWS, the shipped "linear_mid_fill");
  fused  linear_ln on gemm_mid_ln_kernel ("linear_ln_mid" = M, "linear_ln_fill" raised so that every shape from 257 rows is timed);
         "routed" says whether the shipped "linear_ln_fill" takes the shape.
The engine's own flags, row count on the device (m_dev = crops, m_mul = tokens) and output types.  By the method of
tools/mid_gemm_bench.py: every launch of a series on another copy of its weights (LNB_COPIES, default 12), medians over LNB_ROUNDS
interleaved rounds.  Two clocks per arm:
  kernel  the GEMM launch's own dispatch packet (yv_set_launch_timing): the pair's linear alone / the fused kernel;
  step    what one step costs in a stream of dependent launches: a series of LNB_COPIES steps behind a plug that keeps the queue
          full while the host enqueues them, timed by one event pair around the series, divided by its length.  pair step -
          pair kernel is what the LayerNorm launch costs there (its kernel and the dispatch gap).
fused / pair compares the step clocks.  Prints the table and the fill bound it supports."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip
from yvhip import engines

dev = "cuda:0"
COPIES = int(os.environ.get("LNB_COPIES", 12))
ROUNDS = int(os.environ.get("LNB_ROUNDS", 5))
E = yvhip
MODELS = [("vit_base_patch16_224", 768, 197), ("vit_base_patch8_224", 768, 785), ("vit_large_patch16_224", 1024, 197)]
CROPS = (1, 2, 3, 4, 6, 8, 12, 16)
KERNEL = {E.LIN_SKINNY: "skinny", E.LIN_IGEMM: "igemm", E.LIN_DMA: "dma128", E.LIN_P8: "p8", E.LIN_P9: "p9", E.LIN_MID: "mid"}
g = torch.Generator(device=dev).manual_seed(0)
plug_buf = torch.empty(256 << 20, dtype=torch.uint8, device=dev)


def kernel_times(fn, n):
    """Kernel times (us) of the GEMM launch of n steps, from the timestamps of each launch's own dispatch packet."""
    recs = []
    yvhip.reserve_events(2 * n)
    yvhip.LINEAR_HOOK = lambda M, N, K, e0, e1: recs.append((e0, e1))
    try:
        for i in range(n):
            fn(i)
    finally:
        yvhip.LINEAR_HOOK = None
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in recs]


def step_time(fn, n):
    """us per step of a series of n steps enqueued behind a plug (the queue never runs dry while the host enqueues)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        plug_buf.fill_(1)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    keys = ("linear_mid", "linear_mid_fill", "linear_ln_mid", "linear_ln_fill")
    shipped = {k: yvhip.get_option(k) for k in keys}
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {n_cu} CUs; us, medians of {ROUNDS} rounds x {COPIES} launches; shipped linear_ln_fill = "
          f"{shipped['linear_ln_fill']}")
    print(f"# {'model':22s} {'step':9s} {'crops':>5s} {'M':>6s} {'N':>5s} {'tiles128':>8s}  {'pair: route':>11s} {'kernel':>7s} {'step':>7s} "
          f"{'(LN)':>6s}  {'fused: kernel':>13s} {'step':>7s}  fused/pair routed")
    rows = []
    for name, D, tok in MODELS:
        for crops in CROPS:
            M = crops * tok
            cnt = torch.tensor([crops], dtype=torch.int32, device=dev)
            x = torch.randn(M, D, generator=g, device=dev) * 2 + 0.5
            h = torch.zeros(M, D, dtype=torch.bfloat16, device=dev)
            gamma, beta = torch.randn(D, generator=g, device=dev), torch.randn(D, generator=g, device=dev)
            for sname, n, flags in (("norm1-qkv", 3 * D, 0), ("norm2-fc1", 4 * D, E.EPI_GELU)):
                ws = [(torch.randn(n, D, generator=g, device=dev) * 0.05).to(torch.bfloat16) for _ in range(COPIES)]
                bias = torch.randn(n, generator=g, device=dev)
                out = torch.zeros(M, n, dtype=torch.bfloat16, device=dev)
                tiles128 = -(-M // 128) * -(-n // 128)

                def pair(i):
                    yvhip.layernorm(x, gamma, beta, h, M, D, D, D, count_dev=cnt, rows_per_count=tok)
                    yvhip.linear(h, ws[i % COPIES], bias, out, flags=flags, m_dev=cnt, m_mul=tok)

                def fused(i):
                    yvhip.linear_ln(x, gamma, beta, h, ws[i % COPIES], bias, out, flags=flags, m_dev=cnt, m_mul=tok)
                arms = {"pair": (pair, dict(linear_mid=engines.MID_GEMM_ROWS, linear_mid_fill=shipped["linear_mid_fill"], linear_ln_mid=0))}
                routed = False
                if M > 256:
                    arms["fused"] = (fused, dict(linear_ln_mid=M, linear_ln_fill=1 << 20))
                    yvhip.set_option("linear_ln_mid", M)
                    routed = bool(yvhip.linear_ln_route(M, n, D, flags | E.EPI_BIAS).fused)
                    yvhip.set_option("linear_ln_mid", shipped["linear_ln_mid"])
                tk, tsp = {a: [] for a in arms}, {a: [] for a in arms}
                try:
                    for rd in range(ROUNDS + 1):
                        for a, (fn, opts) in arms.items():
                            for key, v in opts.items():
                                yvhip.set_option(key, v)
                            if a == "pair":
                                route = KERNEL[yvhip.linear_route(M, n, D, flags | E.EPI_BIAS, m_dev=True).kernel]
                            else:
                                assert yvhip.linear_ln_route(M, n, D, flags | E.EPI_BIAS).fused == 1
                            k, s = kernel_times(fn, COPIES), step_time(fn, COPIES)
                            if rd:                                  # round 0 warms both arms
                                tk[a] += k
                                tsp[a].append(s)
                            for key, v in shipped.items():
                                yvhip.set_option(key, v)
                finally:
                    for key, v in shipped.items():
                        yvhip.set_option(key, v)
                k = {a: median(v) for a, v in tk.items()}
                s = {a: median(v) for a, v in tsp.items()}
                ratio = s["fused"] / s["pair"] if "fused" in s else None
                rows.append((name, sname, crops, M, n, tiles128, ratio, routed))
                fcell = f"{k['fused']:13.1f} {s['fused']:7.1f}  {ratio:10.2f} {'yes' if routed else 'no'}" if ratio is not None else \
                    f"{'-':>13s} {'-':>7s}  {'-':>10s} no (M <= 256: the pair)"
                print(f"  {name:22s} {sname:9s} {crops:5d} {M:6d} {n:5d} {tiles128:8d}  {route:>11s} {k['pair']:7.1f} {s['pair']:7.1f} "
                      f"{s['pair'] - k['pair']:6.1f}  {fcell}", flush=True)
                del ws, out
    print("#")
    timed = [r for r in rows if r[6] is not None]
    won = sorted({r[5] for r in timed if r[6] <= 1.0})
    lost = sorted({r[5] for r in timed if r[6] > 1.0})
    print(f"# 128 x 128 tile counts at which the fused step was at least as fast: {won}")
    print(f"# ... and at which it was slower: {lost}")
    bound = max([t for t in won if not lost or t < lost[0]], default=0)
    print(f"# every shape up to {bound} tiles of 128 x 128 was at least as fast fused: linear_ln_fill <= {bound * 8 // n_cu} eighths of {n_cu} CUs")
    for r in timed:
        if r[7] and r[6] > 1.0:
            print(f"# routed under the shipped fill but slower fused: {r[:6]} x {r[6]:.2f}")


if __name__ == "__main__":
    main()
