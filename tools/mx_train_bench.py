"""MXFP8 vs bf16 ViT fine-tune step (VitTrainer(dtype="mxfp8") against the default recipe), DESIGN.md section 11.

Both trainers of a shape live in one process and their steps are timed ALTERNATELY (bf16 block, mxfp8 block, repeated
--reps times) with device events around --steps back-to-back steps, after --warmup steps of each: clock and thermal drift
hit both recipes alike.  One JSON line per (model, crops): median step time of each recipe, the speed-up and the model
TFLOP/s (3x the forward's GEMM + attention flops).  Kernel times per role come from a separate rocprofv3 run of one recipe:

    rocprofv3 --kernel-trace --stats -d prof -o mx -- python tools/mx_train_bench.py --only mxfp8 --reps 1
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "yolov8-vit_amd")]

import torch  # noqa: E402


def model_flops(name: str, R: int) -> float:
    from yvhip.engines import vit_cfg
    P, D, L, H = vit_cfg(name)
    tok = (224 // P) ** 2
    N = tok + 1
    M = R * N
    fwd = L * (2 * M * 12 * D * D + 4 * R * N * N * D) + 2 * R * tok * 3 * P * P * D
    return 3.0 * fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="vit_base_patch16_224:32,vit_base_patch16_224:128,vit_large_patch16_224:32")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["bf16", "mxfp8"], default=None, help="one recipe (profiler runs)")
    a = ap.parse_args()
    from yvhip import engines
    from yvhip.training import VitTrainer
    dtypes = [a.only] if a.only else ["bf16", "mxfp8"]
    for spec in a.shapes.split(","):
        name, R = spec.split(":")[0], int(spec.split(":")[1])
        P = engines.vit_cfg(name)[0]
        sd = engines.init_vit_wrapper_state(name, 5, seed=1)
        g = torch.Generator().manual_seed(2)
        pm = (torch.rand(R * (224 // P) ** 2, 3 * P * P, generator=g) * 2 - 1).to(torch.bfloat16).cuda()
        labels = torch.randint(0, 5, (R,), generator=g, dtype=torch.int32).cuda()
        trs = {d: VitTrainer(sd, name, 5, dtype=d) for d in dtypes}
        for d in dtypes:                                          # warm every shape of both recipes
            for _ in range(a.warmup):
                trs[d].step(pm, labels, 1e-4)
        torch.cuda.synchronize()
        times = {d: [] for d in dtypes}
        for _ in range(a.reps):
            for d in dtypes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    trs[d].step(pm, labels, 1e-4)
                e1.record()
                e1.synchronize()
                times[d].append(e0.elapsed_time(e1) / a.steps)
        fl = model_flops(name, R)
        out = {"model": name, "crops": R, "steps": a.steps, "reps": a.reps}
        for d in dtypes:
            ms = statistics.median(times[d])
            out[f"{d}_step_ms"] = round(ms, 3)
            out[f"{d}_step_ms_all"] = [round(t, 3) for t in times[d]]
            out[f"{d}_tflops"] = round(fl / (ms * 1e-3) / 1e12, 1)
        if len(dtypes) == 2:
            out["speedup_mx"] = round(out["bf16_step_ms"] / out["mxfp8_step_ms"], 3)
        print(json.dumps(out), flush=True)
        del trs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
