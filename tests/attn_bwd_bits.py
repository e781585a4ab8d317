"""Recorded bits of the three attention backward entry points (a helper module, like trainer_trace.py; test_gpu_attn_bwd_bits.py is its
test).

The bit tests of test_gpu_attn_long_bwd.py and test_gpu_attn_short_bwd.py compare yv_attention_bwd_long and yv_attention_bwd_short
with yv_attention_bwd.  The three share csrc/attention_bwd_core.h, so a change of that header moves all of them together and those
tests cannot see it.  This fixture can: it holds, per entry point and shape, the sha256 of what the kernels wrote.

Cases: every (R, N, H) of attn_bwd_reference.BWD_SHAPES for attention_bwd and attention_bwd_long, the ones with N <= 224 for
attention_bwd_short: every NT / NW instantiation of the three files at both of its edges.
Inputs: qkv = bf16(randn * 1.5) and dout = bf16(randn) from a CPU generator seeded per shape; out and lse from yv.attention_train on
the device (csrc/attention.hip is bitwise reproducible; a CPU matmul's rounding may depend on the BLAS thread count, so none is used).
Recorded: "operands" = sha256 of the bytes of out then lse; "dqkv" = sha256 of dqkv[:R*N] as little-endian 16-bit words; "delta" =
sha256 of delta_ws[:R*H*N] as little-endian 32-bit words.

The fixture tests/golden/attn_bwd_bits.json is written on an MI355X by `python tests/attn_bwd_bits.py --write [path]`, one line per
case.  Re-record it only with a change that is meant to move the bits, and say so in that change."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

from attn_bwd_reference import BWD_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "attn_bwd_bits.json")
DEV = "cuda:0"
KERNELS = ("attention_bwd", "attention_bwd_long", "attention_bwd_short")
SHORT_MAX = 224                                          # yv_attention_bwd_short refuses more tokens
CASES = [(kern, *s) for kern in KERNELS for s in BWD_SHAPES if kern != "attention_bwd_short" or s[1] <= SHORT_MAX]
PREFILL, TAIL_ROWS, TAIL_FLOATS = 1.5, 64, 64


def case_id(kernel, R, N, H) -> str:
    return f"{kernel}:{R}x{N}x{H}"


def _sha(*tensors) -> str:
    """sha256 of the tensors' raw words (16-bit for bf16, 32-bit for f32; little-endian hosts), in order"""
    h = hashlib.sha256()
    for t in tensors:
        words = t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
        h.update(words.numpy().tobytes())
    return h.hexdigest()


def make_inputs(yv, R, N, H):
    """-> qkv, out, dout, lse on the device (make_inputs of test_gpu_attn_short_bwd.py with a seed per shape)"""
    g = torch.Generator().manual_seed((R * 1009 + N) * 13 + H)
    D = H * 64
    qkv = (torch.randn(R * N, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    dout = torch.randn(R * N, D, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.zeros(R * N, D, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(R * H * N, device=DEV)
    yv.attention_train(qkv, R, N, H, out, lse)
    return qkv, out, dout, lse


def run_case(yv, kernel, R, N, H) -> dict:
    """{"operands", "dqkv", "delta"} hashes of one case and "tail_kept": whether everything past the live rows kept its pre-fill"""
    qkv, out, dout, lse = make_inputs(yv, R, N, H)
    dqkv = torch.full((R * N + TAIL_ROWS, 3 * H * 64), PREFILL, dtype=torch.bfloat16, device=DEV)
    dws = torch.full((R * H * N + TAIL_FLOATS,), PREFILL, device=DEV)
    getattr(yv, kernel)(qkv, out, dout, lse, R, N, H, dqkv, dws)
    torch.cuda.synchronize()
    M, FL = R * N, R * H * N
    return {"operands": _sha(out, lse), "dqkv": _sha(dqkv[:M]), "delta": _sha(dws[:FL]),
            "tail_kept": bool((dqkv[M:] == PREFILL).all()) and bool((dws[FL:] == PREFILL).all())}


def record(yv) -> dict:
    got = {}
    for case in CASES:
        res = run_case(yv, *case)
        assert res.pop("tail_kept"), case
        got[case_id(*case)] = res
    return got


def dumps(cases: dict) -> str:
    """The fixture's text: one line per case."""
    line = lambda v: json.dumps(v, separators=(",", ":"))
    return "{\n" + ",\n".join(f"{line(k)}:{line(v)}" for k, v in cases.items()) + "\n}\n"


def load_fixture() -> dict:
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "yolov8-vit_amd")]
    import yvhip
    yvhip.require_gpu()
    text = dumps(record(yvhip))
    if "--write" in sys.argv[1:]:
        i = sys.argv.index("--write")
        path = sys.argv[i + 1] if len(sys.argv) > i + 1 else FIXTURE
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"wrote {path}: {len(text)} bytes, {text.count(chr(10))} lines")
    else:
        sys.stdout.write(text)
