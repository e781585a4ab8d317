#!/usr/bin/env python3
"""One launch per case of the linears the project makes, for a kernel trace: which kernel, grid, workgroup and LDS size does each
(shape, flags, options) launch?  Two builds that print the same sequence launch the same kernels.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/linear_route_trace.py        # the launches
  python tools/linear_route_trace.py --sequence DIR [--out FILE]     # the (kernel, grid, workgroup, LDS) lines of that trace
  python tools/linear_route_trace.py --sequence DIR --check          # ... each checked against yvhip.linear_route's prediction

Cases: the shapes and flag sets of tests/test_gpu_dense.py, test_gpu_cls_tail.py and test_gpu_mx_train.py, the block linears,
head and trainer forms at the ViT-B/16 bench shapes, and forced variants only where test_gpu_dense.py / tools/gemm_bench.py
force them (a forced instance checks less of the shape than the shipped rule).  The split-K workspace is registered as
yvhip._st() does.  Works on a build without yv_linear_route (no predictions then)."""
import argparse
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, os.environ.get("YV_PKG", "yolov8-vit_amd")))

B, GELU, RES, F32, POS, PRE, GBWD = 1, 4, 8, 32, 64, 128, 256


def cases():
    """(M, N, K, flags, extra, options): extra in {"", "m_dev", "res_f32", "aux", "mx", "mx_res", "mx_aux"}."""
    out = []

    def add(M, N, K, flags, extra="", **opts):
        out.append((M, N, K, flags, extra, opts))

    # tests/test_gpu_dense.py: plain, epilogues, exact-integer (with their device row count runs)
    for M, N, K in ((128, 128, 64), (200, 768, 768), (197 * 3, 2304, 768), (130, 1024, 768), (64, 16, 144), (257, 40, 72), (1000, 64, 576)):
        add(M, N, K, B | F32)
        add(M, N, K, B)
    add(394, 256, 128, B | GELU); add(394, 256, 128, B | RES); add(394, 256, 128, B | F32 | POS); add(394, 256, 128, B | F32, "m_dev")
    exact = ((6304, 768, 768, RES), (6304, 2304, 768, 0), (6304, 3072, 768, GELU), (6304, 768, 3072, RES), (1000, 768, 768, RES),
             (1000, 1000, 768, GELU), (130, 256, 1024, 0), (128 * 70 + 5, 640, 768, GELU), (70000, 384, 768, 0))
    for M, N, K, f in exact:
        add(M, N, K, B | f)
        add(M, N, K, B | f, "m_dev")
    # ... the persistent kernels forced at the shapes and heights of test_linear_persistent_8phase_exact_integer
    forced = ((6304, 2304, 768, 0, 0), (6304, 3072, 768, GELU, 0), (25216, 2304, 768, 0, 0), (25216, 3072, 768, GELU, 256),
              (2048 + 37, 1536, 128, 0, 256), (70000, 256, 192, 0, 0), (12608, 4096, 1024, GELU, 0), (300, 512, 320, 0, 256),
              (25216, 768, 768, RES, 0), (25216, 768, 3072, RES, 0), (12608, 768, 768, RES, 0), (6304, 2304, 768, 0, 128),
              (6304, 768, 768, RES, 160), (6304, 2304, 768, 0, 192), (6304, 3072, 768, GELU, 224), (12608, 768, 3072, RES, 224),
              (5000, 256, 128, F32, 160), (9999, 512, 192, RES, 128), (6304, 768, 768, RES, 96), (6304, 768, 3072, 0, 96),
              (9999, 512, 192, RES, 96), (5000, 256, 128, F32, 96), (300, 512, 320, 0, 128), (70000, 256, 192, GELU, 96),
              (6304, 768, 2304, 0, 0))
    for variant in (9, 11):
        for M, N, K, f, rows in forced:
            add(M, N, K, B | f, linear_variant=variant, linear_p8_rows=rows)
            add(M, N, K, B | f, "m_dev", linear_variant=variant, linear_p8_rows=rows)
    for M, N, K in ((12608, 768, 768), (6304, 2304, 768), (2048 + 37, 1536, 128)):          # the race screen
        for f in (GELU, RES):
            add(M, N, K, B | f, linear_variant=3)
            for cus in (0, 208):
                for rows in (0, 128, 160, 192):
                    add(M, N, K, B | f, linear_variant=9, linear_p8_cus=cus, linear_p8_rows=rows)
    add(2048, 256, 256, GELU, linear_variant=9)                                            # test_gelu_fast_form_accuracy
    for M, N, K, rows in ((6304, 3072, 768, 0), (6304, 768, 3072, 0), (2048 + 37, 768, 256, 160), (6304, 768, 768, 192), (9999, 512, 128, 224)):
        for p8 in (0, 3):                                                                   # the trainer epilogues
            o = dict(linear_p8=p8, linear_p8_rows=rows if p8 else 0)
            add(M, N, K, B | RES, "res_f32", **o); add(M, N, K, B | GELU | PRE, "aux", **o); add(M, N, K, GBWD, "aux", **o)
    # tests/test_gpu_cls_tail.py
    for M in (1, 3, 64, 128, 130, 256):
        for N in (768, 1024, 3072):
            for K in (768, 3072, 1024):
                for f in (0, GELU, RES, F32):
                    add(M, N, K, B | f)
    add(64, 768, 3072, B | RES, "m_dev")
    add(130, 1024, 768, B | F32); add(130, 1024, 768, B | F32, linear_skinny=0)
    # tests/test_gpu_mx_train.py
    mx = (("mx_aux", B | GELU | PRE, 6304, 3072, 768), ("mx_aux", B | GELU | PRE, 6304, 768, 768), ("mx_res", B | RES, 12608, 768, 768),
          ("mx_res", B | RES, 6304, 768, 768), ("mx_aux", GBWD, 6304, 3072, 768), ("mx_aux", GBWD, 1000, 3072, 768),
          ("mx_aux", B | GELU | PRE, 6304, 4096, 1024), ("mx_aux", GBWD, 6304, 4096, 1024), ("mx_aux", B | GELU | PRE, 6304, 3072, 640),
          ("mx_aux", GBWD, 6304, 3072, 640))
    for extra, f, M, N, K in mx:
        add(M, N, K, f, extra)
    for f in (B | GELU | PRE, GBWD):
        for rows in (0, 160, 192, 224):
            add(6304, 3072, 768, f, "mx_aux", linear_p8_rows=rows)
    # the ViT-B/16 bench shapes (64 / 32 crops of 197 tokens; 128 in the R = 128 schedule): qkv, proj, fc1, fc2, head, trainer forms
    for M in (12608, 6304, 25216):
        add(M, 2304, 768, B); add(M, 768, 768, B | RES); add(M, 3072, 768, B | GELU); add(M, 768, 3072, B | RES)
        add(M, 2304, 768, B, "m_dev"); add(M, 768, 768, B | RES, "m_dev"); add(M, 3072, 768, B | GELU, "m_dev"); add(M, 768, 3072, B | RES, "m_dev")
    add(64, 1000, 768, B | F32); add(64, 1008, 768, B | F32, "m_dev")
    for M in (6304, 12608):
        add(M, 768, 768, B | RES, "res_f32"); add(M, 3072, 768, B | GELU | PRE, "aux"); add(M, 768, 3072, B | RES, "res_f32")
        add(M, 768, 3072, 0); add(M, 3072, 768, GBWD, "aux"); add(M, 768, 768, 0); add(M, 768, 2304, 0)      # data gradients
    # tools/gemm_bench.py forces its default variants (3, 10) at these shapes
    for variant in (3, 10):
        for N, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072)):
            add(25216, N, K, B, linear_variant=variant)
    return out


def predicted(yv, M, N, K, flags, extra):
    if not hasattr(yv, "linear_route"):
        return None
    r = yv.linear_route(M, N, K, flags, res_f32=extra in ("res_f32", "mx_res"), ldaux=N if extra in ("aux", "mx_aux") else 0,
                        mx=extra.startswith("mx"), m_dev=extra == "m_dev")
    return r


def kernel_of(r):
    """The substring of the traced kernel name that the route names, and the workgroup size."""
    if r.kernel == 0:
        return "gemm_skinny_kernel", 512
    if r.kernel == 1:
        return f"igemm_kernel<0, 128, {r.tile_cols},", 256
    if r.kernel == 2:
        wg = {(128, 128): 256, (256, 128): 512, (256, 256): 512, (128, 256): 512}[r.tile_rows, r.tile_cols]
        return f"gemm_dma_kernel<{r.tile_rows}, {r.tile_cols}, {'4, 2' if (r.tile_rows, r.tile_cols) == (256, 128) else '2, 2' if wg == 256 else '2, 4'}, {r.abl}, false>", wg
    if r.kernel == 3:
        mf = {128: "2, 2", 160: "3, 2", 192: "3, 3", 224: "4, 3", 256: "4, 4"}[r.tile_rows]
        return f"gemm_p8_kernel<{mf}, {'true' if r.f32out else 'false'}, 0>", 512
    if r.kernel == 4:
        return f"gemm_p9_kernel<{r.tile_rows // 32}, {'true' if r.f32out else 'false'}, 0, {r.ext}, {'true' if r.mx else 'false'}>", 512
    return "gemm_mx_kernel<128, 128, 2, 2>", 256


def launches(args):
    import torch
    import yvhip as yv
    yv.require_gpu()
    dev = "cuda:0"
    log = []
    for i, (M, N, K, flags, extra, opts) in enumerate(cases()):
        old = {k: yv.get_option(k) for k in opts}
        for k, v in opts.items():
            yv.set_option(k, v)
        try:
            r = predicted(yv, M, N, K, flags, extra)
            f32 = bool(flags & (F32 | RES))
            orow = (M // 2) * 3 if flags & POS else M
            out = torch.zeros(orow, N, dtype=torch.float32 if f32 else torch.bfloat16, device=dev)
            bias = torch.zeros(N, device=dev) if flags & B else None
            aux = torch.zeros(M, N, dtype=torch.bfloat16, device=dev) if extra in ("aux", "mx_aux") else None
            res = torch.zeros(M, N, device=dev) if extra in ("res_f32", "mx_res") else None
            fl = flags & ~B
            if extra.startswith("mx"):
                aq = torch.zeros(M, K, dtype=torch.uint8, device=dev); wq = torch.zeros(N, K, dtype=torch.uint8, device=dev)
                sa = torch.full((K // 128, yv.r128(M), 4), 127, dtype=torch.uint8, device=dev)
                sw = torch.full((K // 128, yv.r128(N), 4), 127, dtype=torch.uint8, device=dev)
                yv.linear_mxfp8_ex(aq, sa, wq, sw, bias, out, flags=fl, res_f32=res, aux=aux)
            else:
                a = torch.zeros(M, K, dtype=torch.bfloat16, device=dev); w = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
                if extra in ("res_f32", "aux"):
                    yv.linear_ex(a, w, bias, out, flags=fl, res_f32=res, aux=aux)
                else:
                    md = torch.tensor([M // 3], dtype=torch.int32, device=dev) if extra == "m_dev" else None
                    pos = torch.zeros(3, N, device=dev) if flags & POS else None
                    yv.linear(a, w, bias, out, flags=fl, pos=pos, tok=2 if flags & POS else 0, m_dev=md, m_mul=2)
            torch.cuda.synchronize()
        finally:
            for k, v in old.items():
                yv.set_option(k, v)
        name, wg = kernel_of(r) if r is not None else ("", 0)
        log.append(f"{i}\t{M}\t{N}\t{K}\t{flags}\t{extra or '-'}\t{','.join(f'{k}={v}' for k, v in sorted(opts.items())) or '-'}\t"
                   f"{name}\t{r.grid * wg if r is not None else 0}\t{wg}\t{r.splitk if r is not None else 0}")
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(log) + "\n")
    print(f"{len(log)} cases launched")


GEMM = re.compile(r"gemm_skinny_kernel|igemm_kernel|gemm_dma_kernel|gemm_p8_kernel|gemm_p9_kernel|gemm_mx_kernel|splitk_reduce_kernel")


def sequence(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {d}, found {files}")
    rows = [r for r in csv.DictReader(open(files[0])) if GEMM.search(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::|yvgemm::|^void ", "", r["Kernel_Name"])
        name = re.sub(r"\(.*\)$", "", name).replace(" [clone .kd]", "").strip()
        seq.append((name, int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"]),
                    int(r["Workgroup_Size_X"] if "Workgroup_Size_X" in r else r["Workgroup_Size"]), int(r.get("LDS_Block_Size", -1))))
    return seq


def check(seq, log):
    """Every case's traced launch against the route predicted for it (a split-K case is followed by its reduce pass)."""
    it = iter(seq)
    bad = 0
    for line in open(log):
        i, M, N, K, flags, extra, opts, name, grid, wg, splitk = line.rstrip("\n").split("\t")
        got = next(it)
        if int(splitk) > 1:
            red = next(it)
            if not red[0].startswith("splitk_reduce_kernel"):
                bad += 1; print(f"case {i}: expected the reduce pass, traced {red}")
        if name not in got[0] or (int(grid), int(wg)) != got[1:3]:
            bad += 1; print(f"case {i} ({M} x {N} x {K}, flags {flags}, {extra}, {opts}): predicted {name} grid {grid} wg {wg}, traced {got}")
    rest = list(it)
    if rest:
        bad += 1; print(f"{len(rest)} traced launches beyond the cases")
    print(f"route check: {sum(1 for _ in open(log))} cases, {bad} mismatches")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default="", help="launch mode: write one line per case (with the predicted route) to this file")
    ap.add_argument("--sequence", default="", help="directory of a rocprofv3 kernel trace of a launch-mode run")
    ap.add_argument("--out", default="", help="--sequence: write the sequence here (default: stdout)")
    ap.add_argument("--check", default="", help="--sequence: the --log file of that run; every launch against its predicted route")
    args = ap.parse_args()
    if not args.sequence:
        return launches(args)
    seq = sequence(args.sequence)
    text = "".join(f"{n}\t{g}\t{w}\t{l}\n" for n, g, w, l in seq)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if args.check:
        sys.exit(1 if check(seq, args.check) else 0)


if __name__ == "__main__":
    main()
