#!/usr/bin/env python3
"""Dev tool (GPU box): every Conv entry of detect_launches("n") and ("s") at 1, 2 and 4 images of 640 x 640 and at 1 image of
384 x 640 - the detector as one request runs it - on three routes, interleaved in one process:
  parent  the shipped route ("conv_small" = 0): cgemm_dma_kernel<64, 4, 1, 3> for every layer the step could take;
  s64     cgemm_small_kernel<64, 2> ("conv_small_rows" = 64);
  s32     cgemm_small_kernel<32, 4> ("conv_small_rows" = 32),
the two instances with the M and fill bounds lifted, so that the table covers the shapes the shipped rule leaves out.  Layers that
are not eligible (igemm_kernel's: Cin not a multiple of 64, Cout < 64) are listed with their route and not timed.
By the method of tools/mid_gemm_bench.py: kernel times from the launch's own dispatch packet (yv_set_launch_timing), every launch
of a series on another copy of its weights (CSB_COPIES, default 12), median of the launches of CSB_ROUNDS interleaved rounds.
The engine's own views (channel offsets, pixel strides, upsampled sources, shortcut) and flags; equal launches of a network are
timed once and counted.  "routed": whether the shipped rule (engines.SMALL_MAP_PIXELS, the shipped "conv_small_fill") takes the
layer, and on which instance.  The last lines give, per (tiles of 128 rows, tiles of 64 rows) the ratios, from which the bounds
of conv_route are read, and whether every routed layer is at least as fast as on the parent's route."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolov8-vit_amd"))
import torch
import yvhip
from yvhip import engines

dev = "cuda:0"
COPIES = int(os.environ.get("CSB_COPIES", 12))
ROUNDS = int(os.environ.get("CSB_ROUNDS", 3))
NC = 5
EXTENTS = [(1, 640, 640), (2, 640, 640), (4, 640, 640), (1, 384, 640)]
LIFTED = dict(conv_small=1 << 30, conv_small_fill=1 << 20)
KEYS = ("conv_small", "conv_small_fill", "conv_small_rows")
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, n):
    recs = []
    fn(0); torch.cuda.synchronize()
    yvhip.reserve_events(2 * n)
    yvhip.CONV_HOOK = lambda M, N, e0, e1: recs.append((e0, e1))
    try:
        for i in range(n):
            fn(i)
    finally:
        yvhip.CONV_HOOK = None
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in recs]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def set_options(opts):
    for k, v in opts.items():
        yvhip.set_option(k, v)


def instance(e, B, h, w, ld_out, has_res):
    c = [s[2] for s in e.srcs]
    return yvhip.conv2d_instance(B, h, w, e.k, e.stride, c[0], c[1] if len(c) > 1 else 0, e.cout, ld_out, ld_out if has_res else 0,
                                 e.flags)


def main():
    shipped = {k: yvhip.get_option(k) for k in KEYS}
    routed_opts = dict(shipped, conv_small=engines.SMALL_MAP_PIXELS)
    print(f"# {torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} x {2 * COPIES} launches, routes interleaved")
    print(f"# shipped rule: conv_small = {engines.SMALL_MAP_PIXELS} (engines.SMALL_MAP_PIXELS), conv_small_fill = {shipped['conv_small_fill']}")
    print(f"# {'net':3s} {'B':>1s} {'extent':>7s} {'layer (first of n)':28s} {'n':>2s} {'k':>1s} {'s':>1s} {'cin':>4s} {'cout':>4s} {'M':>6s} "
          f"{'t128':>4s} {'t64':>4s}  {'parent':>7s} {'s64':>7s} {'s32':>7s}  {'s64/p':>5s} {'s32/p':>5s}  routed")
    rows = []
    for scale in ("n", "s"):
        convs = [e for e in engines.detect_launches(scale, NC, True, False) if type(e) is engines.Conv]
        width = {}
        for idx, kind, p in engines.yolo_layers(scale):
            width[f"out{idx}"] = p["cout"]
            if kind == "c2f":
                width[f"y{idx}"], width[f"t{idx}"] = (2 + p["n"]) * (p["cout"] // 2), p["cout"] // 2
            elif kind == "sppf":
                width[f"y{idx}"] = p["cin"] * 2
        _, c2, c3, _ = engines.detect_widths(scale, NC)
        for s in range(3):
            width[f"det{s}.hb"] = width[f"det{s}.hc"] = c2 + c3
        for B, H, W in EXTENTS:
            seen = {}
            for e in convs:
                sig = (e.srcs and tuple((width[b], off, c, up) for b, off, c, up in e.srcs), e.k, e.stride, width[e.out], e.out_off,
                       e.res_off, e.flags, e.cout, e.down)
                if sig in seen:
                    seen[sig][1] += 1
                else:
                    seen[sig] = [e, 1]
            for e, count in seen.values():
                h, w = H // e.down, W // e.down
                M, ld_out = B * h * w, width[e.out]
                set_options(dict(shipped, conv_small=0))
                parent = instance(e, B, h, w, ld_out, e.res_off is not None)
                set_options(dict(LIFTED, conv_small_rows=64))
                eligible = (instance(e, B, h, w, ld_out, e.res_off is not None) & 15) == yvhip.CONV_SMALL_64
                set_options(routed_opts)
                routed = instance(e, B, h, w, ld_out, e.res_off is not None) & 15
                set_options(shipped)
                cin = sum(c for _, _, c, _ in e.srcs)
                head = (f"  {scale:3s} {B:1d} {H:3d}x{W:3d} {e.key:28s} {count:2d} {e.k:1d} {e.stride:1d} {cin:4d} {e.cout:4d} {M:6d} "
                        f"{(M + 127) // 128 * ((e.cout + 63) // 64):4d} {(M + 63) // 64 * ((e.cout + 63) // 64):4d}")
                if not eligible:
                    print(f"{head}  not eligible: route code {parent}", flush=True)
                    continue
                srcs = []
                for b, off, c, up in e.srcs:
                    t = torch.randn(B, (h * e.stride) >> up, (w * e.stride) >> up, width[b], generator=g, device=dev).to(torch.bfloat16)
                    srcs.append(yvhip.view(t, off, c, up))
                K = e.k * e.k * cin
                ws = [(torch.randn(e.cout, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16) for _ in range(COPIES)]
                bias = torch.randn(e.cout, generator=g, device=dev)
                out = torch.zeros(B, h, w, ld_out, dtype=torch.float32 if e.flags & yvhip.EPI_OUT_F32 else torch.bfloat16, device=dev)
                res = out if e.res_off is not None else None
                fn = lambda i: yvhip.conv2d(srcs[0], srcs[1] if len(srcs) > 1 else None, B, h, w, e.k, e.stride, ws[i % COPIES], bias,
                                            out, e.out_off, e.flags, res=res, res_c_off=e.res_off or 0)
                routes = {"parent": dict(shipped, conv_small=0), "s64": dict(LIFTED, conv_small_rows=64),
                          "s32": dict(LIFTED, conv_small_rows=32)}
                ts = {r: [] for r in routes}
                try:
                    for rd in range(ROUNDS):
                        for r, opts in routes.items():
                            set_options(opts)
                            ts[r] += timed(fn, 2 * COPIES)
                finally:
                    set_options(shipped)
                t = {r: median(v) for r, v in ts.items()}
                r64, r32 = t["s64"] / t["parent"], t["s32"] / t["parent"]
                what = {yvhip.CONV_SMALL_64: "s64", yvhip.CONV_SMALL_32: "s32"}.get(routed, "no")
                rows.append((M, (M + 127) // 128 * ((e.cout + 63) // 64), (M + 63) // 64 * ((e.cout + 63) // 64), r64, r32, what, count))
                print(f"{head}  {t['parent']:7.1f} {t['s64']:7.1f} {t['s32']:7.1f}  {r64:5.2f} {r32:5.2f}  {what}", flush=True)
                del srcs, ws, out
    print("#")
    print("# by (128-row tiles, 64-row tiles): s64 / parent and s32 / parent, smallest .. largest over the layers with that count")
    by = {}
    for M, t128, t64, r64, r32, what, count in rows:
        by.setdefault((t128, t64), []).append((r64, r32))
    for (t128, t64), v in sorted(by.items()):
        print(f"#   t128 {t128:4d} t64 {t64:4d}: s64 {min(a for a, _ in v):5.2f} .. {max(a for a, _ in v):5.2f}   "
              f"s32 {min(b for _, b in v):5.2f} .. {max(b for _, b in v):5.2f}   ({len(v)} layers)")
    taken = [(r64 if what == "s64" else r32) for _, _, _, r64, r32, what, _ in rows if what != "no"]
    slower = [x for x in taken if x > 1.0]
    print(f"# the shipped rule takes {len(taken)} of {len(rows)} timed layers; slower than the parent's route: {len(slower)}"
          + (f" (worst x {max(slower):.2f})" if slower else "") + (f"; taken layers x {min(taken):.2f} .. {max(taken):.2f}" if taken else ""))


if __name__ == "__main__":
    main()
