"""Weight gradients of the classifier, 128 x 128 tiles (yv_wgrad: gemm_tn_kernel) against 256 x 128 tiles (yv_wgrad_wide:
gemm_tn_wide_kernel), kernel plus slice reduce, for the dW shapes of ViT-B/16 at 32 / 64 / 128
crops and ViT-L/16 at 64 crops: qkv, proj, fc1, fc2, the head and the patch embedding.  One process; per shape the variants
alternate over ROUNDS rounds of INNER launches after a cache flush, the median round is reported with the rounds' range.

  python tools/wgrad_wide_bench.py [--out FILE]            the table, every variant under its own slice rule
  python tools/wgrad_wide_bench.py slices [--out FILE]     the slice sweep ("wgrad_split" = S) behind the wide tile's slice rule"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolov8-vit_amd"))
import torch
import yvhip

DEV, ROUNDS, INNER = "cuda:0", 7, 10
SWEEP = (1, 2, 3, 4, 5, 6, 8, 9, 12, 16)


def r64(n):
    return (n + 63) // 64 * 64


def vit_shapes(D, crops):
    """(layer, T, N, K) of one block's four linears, the head and the patch embedding (patch 16, 224 x 224: 197 tokens a crop)."""
    T = r64(crops * 197)
    return [("qkv", T, 3 * D, D), ("proj", T, D, D), ("fc1", T, 4 * D, D), ("fc2", T, D, 4 * D), ("head", r64(crops), 1000, D),
            ("patch_embed", r64(crops * 196), D, 768)]


MODELS = (("ViT-B/16", 768, 32), ("ViT-B/16", 768, 64), ("ViT-B/16", 768, 128), ("ViT-L/16", 1024, 64))
VARIANTS = ("128", "wide")


class Shape:
    """Operands of one weight-gradient product: N(0, 1) bf16 (timing does not depend on the values)."""

    def __init__(self, T, N, K, g):
        self.T, self.N, self.K = T, N, K
        self.dy = torch.randn(T, N, generator=g, device=DEV).to(torch.bfloat16)
        self.x = torch.randn(T, K, generator=g, device=DEV).to(torch.bfloat16)
        self.dw = torch.zeros(N, K, device=DEV)

    def route(self, v):
        return yvhip.wgrad_route(self.T, self.N, self.K, 128) if v == "128" else yvhip.wgrad_wide_route(self.T, self.N, self.K)

    def run(self, v):
        if v == "128":
            yvhip.wgrad(self.dy, self.x, self.dw)
        else:
            yvhip.wgrad_wide(self.dy, self.x, self.dw)


def alternate(sh, variants, flush):
    """Median over ROUNDS of the microseconds per launch of each variant, the variants alternating inside every round."""
    ts = {v: [] for v in variants}
    for v in variants:
        sh.run(v)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for v in variants:
            flush.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                sh.run(v)
            e1.record()
            torch.cuda.synchronize()
            ts[v].append(e0.elapsed_time(e1) / INNER * 1e3)
    return {v: sorted(t)[ROUNDS // 2] for v, t in ts.items()}, {v: (min(t), max(t)) for v, t in ts.items()}


def header(what):
    return (f"# python tools/wgrad_wide_bench.py{what}   ({torch.cuda.get_device_name(0)}; us per launch incl. the slice reduce, median "
            f"of {ROUNDS} alternating rounds of {INNER} launches, cache flushed before each round; [min .. max] of the rounds)")


def table(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    flush = torch.zeros(128 * 1024 * 1024, device=DEV)             # 512 MB: past the 256 MB of last-level cache
    lines = [header("")]
    for model, D, crops in MODELS:
        lines.append(f"{model}, {crops} crops")
        lines.append(f"{'layer':12s} {'T':>6s} {'N':>5s} {'K':>5s} | {'128: tiles x S':>14s} {'us':>8s} {'[min .. max]':>17s} | {'wide: tiles x S':>15s} "
                     f"{'us':>8s} {'[min .. max]':>17s} | wide / 128  routed tile")
        for layer, T, N, K in vit_shapes(D, crops):
            sh = Shape(T, N, K, g)
            r0, r1 = sh.route("128"), sh.route("wide")
            med, rng = alternate(sh, VARIANTS, flush)
            routed = yvhip.wgrad_wide_route(T, N, K, routed=True).tile_n
            lines.append(f"{layer:12s} {T:6d} {N:5d} {K:5d} | {r0.tiles:8d} x {r0.slices:3d} {med['128']:8.1f} [{rng['128'][0]:6.1f} .. {rng['128'][1]:6.1f}] | "
                         f"{r1.tiles:9d} x {r1.slices:3d} {med['wide']:8.1f} [{rng['wide'][0]:6.1f} .. {rng['wide'][1]:6.1f}] | "
                         f"{med['wide'] / med['128']:10.3f}  {routed:11d}")
            del sh
            print(lines[-1], flush=True)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


def slices(out):
    """Every variant at forced slice counts; a count the workspace does not hold is reported as the count that ran."""
    g = torch.Generator(device=DEV).manual_seed(0)
    flush = torch.zeros(128 * 1024 * 1024, device=DEV)
    lines = [header(" slices")]
    try:
        for model, D, crops in (MODELS[0], MODELS[2]):
            lines.append(f"{model}, {crops} crops: us at \"wgrad_split\" = S (S as launched); rule = the variant's own slice rule")
            for layer, T, N, K in vit_shapes(D, crops)[:4]:
                sh = Shape(T, N, K, g)
                for v in VARIANTS:
                    yvhip.set_option("wgrad_split", 0)
                    own = sh.route(v).slices
                    cells = []
                    for S in SWEEP + (0,):
                        yvhip.set_option("wgrad_split", S)
                        ran = sh.route(v).slices
                        if S and ran != S:
                            continue
                        med, _ = alternate(sh, [v], flush)
                        cells.append(f"{'rule=' + str(ran) if not S else S}: {med[v]:6.1f}")
                    lines.append(f"{layer:6s} {T:6d} {N:5d} {K:5d} {v:6s} (rule S = {own:2d}) | " + "  ".join(cells))
                    print(lines[-1], flush=True)
                del sh
    finally:
        yvhip.set_option("wgrad_split", 0)
    if out:
        open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    yvhip.require_gpu()
    args = sys.argv[1:]
    mode = slices if args[:1] == ["slices"] else table
    args = args[1:] if args[:1] == ["slices"] else args
    mode(args[1] if args[:1] == ["--out"] else None)
