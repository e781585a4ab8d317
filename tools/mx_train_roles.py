"""Kernel time of a `rocprofv3 --kernel-trace` run of tools/mx_train_bench.py (rocpd SQLite output), per kernel and per role
of the fine-tune step: forward + data-gradient GEMMs, weight-gradient GEMMs (+ their split-K reduce), quantisation passes,
everything else.  The weight gradients of the transformer blocks run on the trainer's side stream, which is how a launch of the
MX kernel that serves both roles is told apart (any shape).  Per-step figures divide by the number of trainer steps the run made (--steps-run).

    python tools/mx_train_roles.py prof/mx_results.db --steps-run 15 --csv profiles/mx_train_kernel_stats_mxfp8.csv
"""
import argparse
import csv
import sqlite3
from collections import defaultdict

WGRAD_BF16 = ("gemm_tn_kernel",)


def role(name: str, side: bool) -> str:
    """Role of a kernel launch; `side`: launched on the trainer's weight-gradient stream (any stream but the one that runs the
    attention backward).  Shape-independent: a gemm_mx_kernel launch is a weight gradient exactly when it runs there."""
    if "quant_mx" in name:
        return "quantisation"
    if "splitk_reduce_kernel" in name or any(k in name for k in WGRAD_BF16):
        return "weight-gradient GEMM"
    if "gemm_mx_kernel" in name:
        return "weight-gradient GEMM" if side else "forward + data-gradient GEMM"
    if "gemm_p9_kernel" in name or "gemm_dma_kernel" in name or "gemm_p8_kernel" in name:
        return "forward + data-gradient GEMM"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--steps-run", type=int, default=15)
    ap.add_argument("--csv", default=None)
    a = ap.parse_args()
    c = sqlite3.connect(a.db)
    rows = c.execute("select name, duration, stream_id from kernels").fetchall()
    main_streams = {sid for name, _, sid in rows if "attn_bwd" in name}
    per = defaultdict(lambda: [0, 0])
    roles = defaultdict(int)
    total = 0
    for name, dur, sid in rows:
        if name.startswith("__amd"):
            continue
        short = name.replace("yvgemm::", "").replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0]
        per[short][0] += 1
        per[short][1] += dur
        roles[role(short, sid not in main_streams)] += dur
        total += dur
    ranked = sorted(per.items(), key=lambda kv: -kv[1][1])
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage"])
            for k, (n, d) in ranked:
                w.writerow([k, n, d, round(d / n, 1), round(100.0 * d / total, 2)])
    print(f"kernel time {total / 1e6:.2f} ms over {a.steps_run} steps = {total / 1e6 / a.steps_run:.3f} ms per step")
    for r, d in sorted(roles.items(), key=lambda kv: -kv[1]):
        print(f"  {r:32s} {d / 1e3 / a.steps_run:9.1f} us per step  {100.0 * d / total:5.1f} %")
    for k, (n, d) in ranked[:12]:
        print(f"  {d / 1e3 / a.steps_run:9.1f} us/step {n / a.steps_run:6.1f} calls/step  {k[:110]}")


if __name__ == "__main__":
    main()
