#!/usr/bin/env python3
"""Dev tool (GPU box): the four block products of ViT-B/16, ViT-B/8 and ViT-L/16 at 1, 2, 4, 8, 16, 32 crops - the classifier as
DetectClassifyPipeline(fit_crops=True) sizes it - on three routes, interleaved in one process:
  parent  the shipped route ("linear_mid" = 0): skinny up to 256 rows, 128 x 128 LDS-DMA tiles, the persistent kernel from 2,048;
  mid     gemm_mid_kernel ("linear_mid" = M), from 257 rows up to MGB_MID_MAX; "routed" says whether the route step takes the shape
          under the shipped "linear_mid_fill" (no: it is timed with the fill rule lifted, and ships on the parent's route);
  skinny  gemm_skinny_kernel with "linear_skinny" raised to M (up to MGB_SKINNY_MAX rows): whether a new kernel was needed.
The engine's own flags, row count on the device (m_dev = crops, m_mul = tokens) and output types.  By the method of
tools/tail_bench.py: kernel times from the launch's own dispatch packet (yv_set_launch_timing), every launch of a series on
another copy of its weights (MGB_COPIES, default 12), median of the launches of MGB_ROUNDS interleaved rounds.
Prints the table and, per model and over all, the largest M up to which every product the route step takes is at least as fast
on the mid kernel as on the parent's route (the bound "linear_mid" ships with is at most 4,096).
--mx: the same models, products and crop counts for an mxfp8 engine (linear_mxfp8; fc1 as linear_mxfp8_q, its fc1 -> fc2 hand-over)
on two routes: parent ("linear_mx_mid" = 0: gemm_mx_kernel 128 x 128, the persistent kernel where its rule takes the shape) and
mid (gemm_mx_mid_kernel, "linear_mx_mid" = M, from one row on), measured the same way; the column "tiles" is the count of
128 x 128 tiles "linear_mx_mid_fill" is compared with (tiles * 8 <= fill * CUs)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip

dev = "cuda:0"
COPIES = int(os.environ.get("MGB_COPIES", 12))
ROUNDS = int(os.environ.get("MGB_ROUNDS", 3))
MID_MAX = int(os.environ.get("MGB_MID_MAX", 8192))          # rows up to which the mid route is timed
SKINNY_MAX = int(os.environ.get("MGB_SKINNY_MAX", 4096))
E = yvhip
MODELS = [("vit_base_patch16_224", 768, 197), ("vit_base_patch8_224", 768, 785), ("vit_large_patch16_224", 1024, 197)]
CROPS = (1, 2, 4, 8, 16, 32)
KERNEL = {E.LIN_SKINNY: "skinny", E.LIN_IGEMM: "igemm", E.LIN_DMA: "dma128", E.LIN_P8: "p8", E.LIN_P9: "p9", E.LIN_MID: "mid"}
g = torch.Generator(device=dev).manual_seed(0)          # operands are made on the device: the host's generator would be most of the run


def timed_linear(fn, n):
    """Kernel times (us) of n launches, from the start / stop timestamps of each launch's own dispatch packet."""
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
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in recs]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    shipped = {k: yvhip.get_option(k) for k in ("linear_mid", "linear_skinny", "linear_mid_fill")}
    print(f"# {torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} x {2 * COPIES} launches; mid / parent in the last column")
    print(f"# {'model':22s} {'product':5s} {'crops':>5s} {'M':>6s} {'N':>5s} {'K':>5s}  {'parent':>16s} {'mid':>8s} {'skinny':>8s}  mid/parent routed")
    ok_to = {}                                              # model -> {M: every product the step takes is at least as fast}
    for name, D, tok in MODELS:
        products = [("qkv", 3 * D, D, 0, torch.bfloat16), ("proj", D, D, E.EPI_RES_F32, torch.float32),
                    ("fc1", 4 * D, D, E.EPI_GELU, torch.bfloat16), ("fc2", D, 4 * D, E.EPI_RES_F32, torch.float32)]
        ok_to[name] = {}
        for crops in CROPS:
            M = crops * tok
            cnt = torch.tensor([crops], dtype=torch.int32, device=dev)
            for pname, n, k, flags, odt in products:
                a = torch.randn(M, k, generator=g, device=dev).to(torch.bfloat16)
                ws = [(torch.randn(n, k, generator=g, device=dev) * 0.05).to(torch.bfloat16) for _ in range(COPIES)]
                bias = torch.randn(n, generator=g, device=dev)
                out = torch.zeros(M, n, dtype=odt, device=dev)
                fill = shipped["linear_mid_fill"]
                routes = {"parent": dict(linear_mid=0, linear_skinny=shipped["linear_skinny"], linear_mid_fill=fill)}
                if 256 < M <= MID_MAX:
                    routes["mid"] = dict(linear_mid=M, linear_skinny=shipped["linear_skinny"], linear_mid_fill=1 << 20)
                    yvhip.set_option("linear_mid", M)
                    routed = yvhip.linear_route(M, n, k, flags | E.EPI_BIAS, m_dev=True).kernel == E.LIN_MID
                    yvhip.set_option("linear_mid", shipped["linear_mid"])
                if 256 < M <= SKINNY_MAX:
                    routes["skinny"] = dict(linear_mid=0, linear_skinny=M, linear_mid_fill=fill)
                ts = {r: [] for r in routes}
                kern = {}
                try:
                    for rd in range(ROUNDS):
                        for r, opts in routes.items():
                            for key, v in opts.items():
                                yvhip.set_option(key, v)
                            kern[r] = KERNEL[yvhip.linear_route(M, n, k, flags | E.EPI_BIAS, m_dev=True).kernel]
                            ts[r] += timed_linear(lambda i: yvhip.linear(a, ws[i % COPIES], bias, out, flags=flags, m_dev=cnt,
                                                                         m_mul=tok), 2 * COPIES)
                finally:
                    for key, v in shipped.items():
                        yvhip.set_option(key, v)
                assert kern.get("mid", "mid") == "mid" and kern.get("skinny", "skinny") == "skinny", kern
                t = {r: median(v) for r, v in ts.items()}
                ratio = t["mid"] / t["parent"] if "mid" in t else None
                if ratio is not None and routed:
                    ok_to[name][M] = ok_to[name].get(M, True) and ratio <= 1.0
                cell = lambda r: f"{t[r]:8.1f}" if r in t else f"{'-':>8s}"
                print(f"  {name:22s} {pname:5s} {crops:5d} {M:6d} {n:5d} {k:5d}  {t['parent']:8.1f} {kern['parent']:>7s} {cell('mid')} "
                      f"{cell('skinny')}  {'' if ratio is None else f'{ratio:6.2f}     ' + ('yes' if routed else 'no')}", flush=True)
                del a, ws, out
    print("#")
    for name, D, tok in MODELS:
        won = [M for M, ok in sorted(ok_to[name].items()) if ok]
        lost = [M for M, ok in sorted(ok_to[name].items()) if not ok]
        print(f"# {name}: the route step takes products at M = {sorted(ok_to[name])}; every one at least as fast at {won}, not at {lost}")
    every = sorted({M for d in ok_to.values() for M in d})
    bad = [M for M in every if not all(d.get(M, True) for d in ok_to.values())]
    good = [M for M in every if not bad or M < bad[0]]
    print(f"# all models: every product the step takes is at least as fast up to M = {max(good) if good else 0} "
          f"(largest M measured with such a product: {max(every) if every else 0}; the bound is at most 4,096)")

def main_mx():
    keys = ("linear_mx_mid", "linear_mx_mid_fill")
    shipped = {k: yvhip.get_option(k) for k in keys}
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    kname = {**KERNEL, E.LIN_MX: "mx128", E.LIN_MX_MID: "mxmid"}
    print(f"# {torch.cuda.get_device_name(0)}, {n_cu} CUs; MXFP8 operands; us per launch, median of {ROUNDS} x {2 * COPIES} launches; "
          f"mid / parent in the last columns; shipped linear_mx_mid_fill = {shipped['linear_mx_mid_fill']}")
    print(f"# {'model':22s} {'product':5s} {'crops':>5s} {'M':>6s} {'N':>5s} {'K':>5s} {'tiles':>5s}  {'parent':>16s} {'mid':>8s}  mid/parent routed")
    rows = []                                                # (tiles, M, ratio, routed)
    for name, D, tok in MODELS:
        products = [("qkv", 3 * D, D, 0, torch.bfloat16, False), ("proj", D, D, E.EPI_RES_F32, torch.float32, False),
                    ("fc1", 4 * D, D, E.EPI_GELU, None, True), ("fc2", D, 4 * D, E.EPI_RES_F32, torch.float32, False)]
        for crops in CROPS:
            M = crops * tok
            cnt = torch.tensor([crops], dtype=torch.int32, device=dev)
            for pname, n, k, flags, odt, qform in products:
                aq, asc = yvhip.quant_mxfp8(torch.randn(M, k, generator=g, device=dev).to(torch.bfloat16))
                ws = [yvhip.quant_mxfp8((torch.randn(n, k, generator=g, device=dev) * 0.05).to(torch.bfloat16)) for _ in range(COPIES)]
                bias = torch.randn(n, generator=g, device=dev)
                if qform:
                    oq = torch.zeros(M, n, dtype=torch.uint8, device=dev)
                    osc = torch.zeros(n // 128, (M + 255) // 256 * 256, 4, dtype=torch.uint8, device=dev)
                    call = lambda i: yvhip.linear_mxfp8_q(aq, asc, ws[i % COPIES][0], ws[i % COPIES][1], bias, oq, osc, flags=flags,
                                                          m_dev=cnt, m_mul=tok)
                    route = lambda: yvhip.linear_mxfp8_q_route(M, n, k, flags | E.EPI_BIAS, m_dev=True)
                else:
                    out = torch.zeros(M, n, dtype=odt, device=dev)
                    call = lambda i: yvhip.linear_mxfp8(aq, asc, ws[i % COPIES][0], ws[i % COPIES][1], bias, out, flags=flags,
                                                        m_dev=cnt, m_mul=tok)
                    route = lambda: yvhip.linear_route(M, n, k, flags | E.EPI_BIAS, mx=True, m_dev=True)
                routes = {"parent": dict(linear_mx_mid=0, linear_mx_mid_fill=shipped["linear_mx_mid_fill"])}
                routed = False
                if M <= MID_MAX:
                    routes["mid"] = dict(linear_mx_mid=M, linear_mx_mid_fill=1 << 20)
                    yvhip.set_option("linear_mx_mid", M)
                    routed = route().kernel == E.LIN_MX_MID
                    yvhip.set_option("linear_mx_mid", shipped["linear_mx_mid"])
                ts = {r: [] for r in routes}
                kern = {}
                try:
                    for rd in range(ROUNDS):
                        for r, opts in routes.items():
                            for key, v in opts.items():
                                yvhip.set_option(key, v)
                            kern[r] = kname[route().kernel]
                            ts[r] += timed_linear(call, 2 * COPIES)
                finally:
                    for key, v in shipped.items():
                        yvhip.set_option(key, v)
                assert kern.get("mid", "mxmid") == "mxmid" and kern["parent"] in ("mx128", "p9"), kern
                t = {r: median(v) for r, v in ts.items()}
                tiles = ((M + 127) // 128) * ((n + 127) // 128)
                ratio = t["mid"] / t["parent"] if "mid" in t else None
                if ratio is not None:
                    rows.append((tiles, M, ratio, routed))
                mid = f"{t['mid']:8.1f}" if "mid" in t else f"{'-':>8s}"
                print(f"  {name:22s} {pname:5s} {crops:5d} {M:6d} {n:5d} {k:5d} {tiles:5d}  {t['parent']:8.1f} {kern['parent']:>7s} {mid}  "
                      f"{'' if ratio is None else f'{ratio:6.2f}     ' + ('yes' if routed else 'no')}", flush=True)
                del aq, asc, ws
    print("#")
    rows.sort()
    lost = [r for r in rows if r[2] > 1.0]
    first_lost = lost[0][0] if lost else None
    won_to = max([r[0] for r in rows if first_lost is None or r[0] < first_lost], default=0)
    fill = (first_lost * 8 - 1) // n_cu if lost else 1 << 20    # the largest fill that admits no product measured slower
    print(f"# {len(rows)} products timed on both routes; mid at least as fast at every product of up to {won_to} tiles"
          + (f", slower first at {first_lost} tiles: the largest fill that takes none measured slower is {fill} eighths of {n_cu} CUs "
             f"(up to {fill * n_cu // 8} tiles)" if lost else "; slower nowhere"))
    good_m = max([r[1] for r in rows if r[0] * 8 <= fill * n_cu], default=0)
    print(f"# under that fill the largest M with a product the step takes: {good_m}")
    print(f"# products measured slower on mid: {[(tl, M, round(x, 2)) for tl, M, x, _ in lost]}")
    taken = [r for r in rows if r[3]]
    print(f"# under the shipped fill the step takes {len(taken)} of them; slower among those: {[(tl, M, round(x, 2)) for tl, M, x, _ in taken if x > 1.0]}")


if __name__ == "__main__":
    main_mx() if "--mx" in sys.argv[1:] else main()
