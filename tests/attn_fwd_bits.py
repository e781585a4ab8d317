"""Recorded bits of the attention forward entry points (a helper module, like attn_bwd_bits.py; test_gpu_attn_fwd_bits.py is its
test, test_attn_fwd_bits_cpu.py checks the fixture's shape without a device).

The bit tests of test_gpu_fp8.py and test_gpu_attn_long.py compare yv_attention_mxfp8 with yv_attention followed by the quantiser and
yv_attention_long with yv_attention.  The three kernel families (attention_kernel, attention_pipe_kernel, attention_long_kernel)
share csrc/attention_fwd_core.h, so a change of that header moves all of them together and those tests cannot see it.  This fixture
can: it holds, per entry point, output form and shape, the sha256 of what the kernels wrote.

Cases (R = 2, H = 2 unless stated: every kernel instance at both of its edges):
  attention, attention_train, attention_mxfp8 on the default route: attention_pipe_kernel<1..7> at N = 32 NT - 31 and 32 NT (and 197),
      attention_kernel<8, 0, true> at 225 and 256, attention_kernel<8, 0, false> at 257 (a one-key second tile), 512, 513, 785; one
      odd head count, (1, 197, 3), without the MX form (it wants H even).
  attention under yv_attention_debug(5): the one-item form attention_kernel<NT, 0, true>, NT = 1..7, which production launches when the
      qkv tensor passes 2 GB; under yv_attention_debug(4): the held-groups form attention_kernel<NT, 0, false> at one tile.
  attention_long in its three output forms (out; out + lse; the MX image alone, out = None): no full 128-query block with a remainder
      launch of 1..4 waves, one full block with and without remainder, the one-wave 32-key-tile workgroup, the ViT lengths.
Inputs: qkv = bf16(randn * 1.5) from a CPU generator seeded by the case id.  Nothing is computed by a CPU matmul, whose rounding may
depend on the BLAS thread count.  Every output buffer is pre-filled with a sentinel and carries TAIL_ROWS spare rows.
Recorded: "bits" = sha256 of, in order: out[:R*N] (16-bit words); lse[:R*H*N] (32-bit words); the e4m3 bytes of the R*N live rows;
the whole scale array, sentinel included - whichever of them the form writes.  Checked besides: "tail_kept", everything past the live
rows kept its pre-fill.

The fixture tests/golden/attn_fwd_bits.json is written on an MI355X by `python tests/attn_fwd_bits.py --write [path]`, one line per
case.  It was recorded from the library of commit 39d40ed, the last one with a separate text of the arithmetic per kernel family.
Re-record it only with a change that is meant to move the bits, and say so in that change."""
from __future__ import annotations

import hashlib
import json
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "attn_fwd_bits.json")
DEV = "cuda:0"
FIELDS = ("bits",)
PREFILL, SENT_Q, SENT_S, TAIL_ROWS = 1.5, 0xA5, 0x5B, 64

EDGES = [n for nt in range(1, 8) for n in (32 * nt - 31, 32 * nt)]                      # 1, 32, 33, 64, ..., 193, 224
DEFAULT_N = sorted(EDGES + [197]) + [225, 256] + [257, 512, 513, 785]
LONG_N = EDGES + [225, 256, 257, 577, 785]
DEFAULT_FORMS = ("attention", "attention_train", "attention_mxfp8")
LONG_FORMS = ("attention_long:out", "attention_long:out+lse", "attention_long:mx")

# (form, yv_attention_debug value, R, N, H)
CASES = [(form, 0, 2, N, 2) for form in DEFAULT_FORMS for N in DEFAULT_N]
CASES += [(form, 0, 1, 197, 3) for form in ("attention", "attention_train")]
CASES += [("attention", 5, 2, N, 2) for N in EDGES]
CASES += [("attention", 4, 2, N, 2) for N in (33, 197)]
CASES += [(form, 0, 2, N, 2) for form in LONG_FORMS for N in LONG_N]


def case_id(form, debug, R, N, H) -> str:
    return f"{form}:{R}x{N}x{H}" + (f":debug{debug}" if debug else "")


def _sha(*tensors) -> str:
    """sha256 of the tensors' raw words (bytes, 16-bit for bf16, 32-bit for f32; little-endian hosts), in order"""
    h = hashlib.sha256()
    for t in tensors:
        words = t.detach().cpu().contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])
        h.update(words.numpy().tobytes())
    return h.hexdigest()


def _launch(yv, form, qkv, R, N, H, out, lse, q, s):
    if form == "attention":
        yv.attention(qkv, R, N, H, out)
    elif form == "attention_train":
        yv.attention_train(qkv, R, N, H, out, lse)
    elif form == "attention_mxfp8":
        yv.attention_mxfp8(qkv, R, N, H, q, s)
    else:
        yv.attention_long(qkv, R, N, H, out, lse=lse, out_q=q, out_scale=s)


def run_case(yv, form, debug, R, N, H) -> dict:
    """{"bits": hash of what the form wrote} of one case and "tail_kept": whether everything past the live rows kept its pre-fill"""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(form, debug, R, N, H).encode()))
    D, M, FL = H * 64, R * N, R * H * N
    qkv = (torch.randn(M, 3 * D, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    has_out = form in ("attention", "attention_train", "attention_long:out", "attention_long:out+lse")
    has_lse = form in ("attention_train", "attention_long:out+lse")
    has_mx = form in ("attention_mxfp8", "attention_long:mx")
    out = torch.full((M + TAIL_ROWS, D), PREFILL, dtype=torch.bfloat16, device=DEV) if has_out else None
    lse = torch.full((FL + TAIL_ROWS,), PREFILL, device=DEV) if has_lse else None
    q = torch.full((M + TAIL_ROWS, D), SENT_Q, dtype=torch.uint8, device=DEV) if has_mx else None
    s = torch.full((D // 128, (M + TAIL_ROWS + 127) // 128 * 128, 4), SENT_S, dtype=torch.uint8, device=DEV) if has_mx else None
    if debug:
        assert yv.lib.yv_attention_debug(debug) == 0
    try:
        _launch(yv, form, qkv, R, N, H, out, lse, q, s)
        torch.cuda.synchronize()
    finally:
        if debug:
            assert yv.lib.yv_attention_debug(0) == 0
    hashed, kept = [], True
    if has_out:
        hashed.append(out[:M])
        kept = kept and bool((out[M:] == PREFILL).all())
    if has_lse:
        hashed.append(lse[:FL])
        kept = kept and bool((lse[FL:] == PREFILL).all())
    if has_mx:
        hashed += [q[:M], s]
        kept = kept and bool((q[M:] == SENT_Q).all()) and bool((s[:, M:] == SENT_S).all())
    return {"bits": _sha(*hashed), "tail_kept": kept}


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
