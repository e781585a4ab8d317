"""Recorded bits of the weight-gradient ("TN") GEMM entry points (a helper module, like attn_bwd_bits.py; test_gpu_wgrad_bits.py is
its test).

The bit tests of test_gpu_wgrad_narrow.py, test_gpu_wgrad_wide.py and test_gpu_wgrad_gather.py compare the narrow, wide and gather
tiles with the 128 x 128 tile.  All of them are instances of one device text (gemm_tn_body in csrc/gemm.hip), so a change of that
text moves them together and those tests cannot see it.  This fixture can: it holds, per entry point, tile and shape, the sha256 of the dW written.

Cases (every instance of the text, at both of its edges; each asserts its route - tile_n and slices - before it launches):
  wgrad_tiled        tile 128 / 64 / 32; (N, K) corners of test_gpu_wgrad_narrow.py; T = 64 (one token tile, nothing in flight), 192
                     (odd tile count, one slice), 1088 (two slices of 8 and 9 tiles through the stream's workspace); dY and X are
                     column windows of wider buffers.
  wgrad_wide         the 256 x 128 tile (mode 1); one to three n and k tiles; T as above (1088: eight slices), T = 192 in two forced
                     slices, and (1088, 1032, 648) in the default eight and in three forced slices, neither of which divides 17.
  wgrad_conv3_tiled  segment addressing of X on the zero-padded pixel grid; tile 128 / 64 / 32; the grids of
                     test_wgrad_conv3_tiled_exact.
  wgrad_conv3_gather gathered source addresses; tile 128 / 64 / 32; the SHAPES of test_gpu_wgrad_gather.py, operands as channel
                     slices of wider buffers.
Inputs: N(0, 1) rounded to bf16 from a CPU generator seeded per case (zeros where the entry point's contract wants zeros).  Nothing
is computed by a CPU matmul, whose rounding may depend on the BLAS thread count.
Recorded: "dw" = sha256 of the dW window as little-endian 32-bit words.  Checked besides: "tail_kept", the sentinel that surrounds
the window is untouched.

The fixture tests/golden/wgrad_bits.json is written on an MI355X by `python tests/wgrad_bits.py --write [path]`, one line per
case.  It was recorded from the library of commit dcbfc38, the last one with a separate text per tile shape.  Re-record it only with
a change that is meant to move the bits, and say so in that change."""
from __future__ import annotations

import contextlib
import hashlib
import json
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "wgrad_bits.json")
DEV = "cuda:0"
SENT, OFF, WOFF = -77.0, 8, 8                            # pre-fill of dW's buffer; column offset of the operands / of dW in theirs
TILES = (128, 64, 32)
TS = (64, 192, 1088)
NARROW_NK = ((8, 8), (24, 72), (40, 264), (72, 576), (80, 576))
WIDE_NK = ((8, 8), (136, 72), (264, 136), (520, 264))
UNEVEN = (1088, 1032, 648)
CONV3_GRIDS, CONV3_CH = ((2, 8), (1, 12)), ((8, 16), (64, 64))          # (B, H); (Cin, Cout)
GATHER_SHAPES = (((1, 6, 6, 2), 8, 16), ((2, 24, 20, 2), 24, 40), ((2, 7, 5, 2), 32, 8), ((3, 16, 16, 2), 136, 136),
                 ((2, 9, 8, 1), 16, 64))                                # (B, Hin, Win, stride), Cin, N

# (entry, tile_n, shape, wgrad_split, expected slices)
CASES = [("wgrad_tiled", t, (T, N, K), 0, 2 if T == 1088 else 1) for t in TILES for N, K in NARROW_NK for T in TS]
CASES += [("wgrad_wide", 256, (T, N, K), 0, 8 if T == 1088 else 1) for N, K in WIDE_NK for T in TS]
CASES += [("wgrad_wide", 256, (192, N, K), 2, 2) for N, K in WIDE_NK]
CASES += [("wgrad_wide", 256, UNEVEN, 0, 8), ("wgrad_wide", 256, UNEVEN, 3, 3)]
CASES += [("wgrad_conv3_tiled", t, (B, H, Cin, Cout), 0, 1) for t in TILES for B, H in CONV3_GRIDS for Cin, Cout in CONV3_CH]
CASES += [("wgrad_conv3_gather", t, (*grid, Cin, N), 0, 1) for t in TILES for grid, Cin, N in GATHER_SHAPES]


def case_id(entry, tile_n, shape, split, slices) -> str:
    return f"{entry}:tile{tile_n}:{'x'.join(map(str, shape))}" + (f":split{split}" if split else "")


def r64(n):
    return (n + 63) // 64 * 64


def _sha(t) -> str:
    """sha256 of an f32 tensor's words (little-endian hosts)"""
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.int32).numpy().tobytes()).hexdigest()


def _normal(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16)


@contextlib.contextmanager
def _split(yv, split):
    old = yv.get_option("wgrad_split")
    try:
        yv.set_option("wgrad_split", split)
        yield
    finally:
        yv.set_option("wgrad_split", old)


def _window(N, K):
    """-> (dW window, the wider sentinel-filled tensor it lives in)"""
    wb = torch.full((N + 8, K + 24), SENT, device=DEV)
    return wb[:N, WOFF:WOFF + K], wb


def _matrix(yv, g, entry, tile_n, shape, slices):
    T, N, K = shape
    route = yv.wgrad_wide_route(T, N, K) if entry == "wgrad_wide" else yv.wgrad_route(T, N, K, tile_n)
    assert (route.tile_n, route.slices) == (tile_n, slices), route
    yb, xb = _normal(g, T, N + 16).to(DEV), _normal(g, T, K + 16).to(DEV)
    dw, wb = _window(N, K)
    if entry == "wgrad_wide":
        yv.wgrad_wide(yb[:, :N], xb[:, OFF:OFF + K], dw)
    else:
        yv.wgrad(yb[:, :N], xb[:, OFF:OFF + K], dw, tile_n=tile_n)
    return dw, wb


def _conv3(yv, g, tile_n, shape, slices):
    """Operands over the zero-padded pixel grid, built on the host: zero ring in both, zero tail rows in dY; the margin and the
    tail rows of the activation hold finite values that the zero rows of dY multiply."""
    B, H, Cin, Cout = shape
    hp = H + 2
    tpad, mg = B * hp * hp, hp + 1
    tpp = r64(tpad)
    route = yv.wgrad_route(tpp, Cout, 9 * Cin, tile_n)
    assert (route.tile_n, route.slices) == (tile_n, slices), route
    buf = _normal(g, tpp + 2 * mg, Cin)
    x = torch.zeros(B, hp, hp, Cin, dtype=torch.bfloat16)
    x[:, 1:-1, 1:-1] = _normal(g, B, H, H, Cin)
    buf[mg:mg + tpad] = x.view(tpad, Cin)
    dy = torch.zeros(B, hp, hp, Cout, dtype=torch.bfloat16)
    dy[:, 1:-1, 1:-1] = _normal(g, B, H, H, Cout)
    dyp = torch.zeros(tpp, Cout, dtype=torch.bfloat16)
    dyp[:tpad] = dy.view(tpad, Cout)
    buf = buf.to(DEV)
    dw, wb = _window(Cout, 9 * Cin)
    yv.wgrad_conv3(dyp.to(DEV), buf[mg:mg + tpp], dw, tpp, hp, tile_n=tile_n)
    return dw, wb


def _gather(yv, g, tile_n, shape, slices):
    B, Hin, Win, stride, Cin, N = shape
    T = B * ((Hin - 1) // stride + 1) * ((Win - 1) // stride + 1)
    route, _ = yv.wgrad_conv3_gather_route(B, Hin, Win, stride, Cin, N, tile_n)
    assert (route.tile_n, route.slices) == (tile_n, slices), route
    xb = _normal(g, B * Hin * Win, Cin + 24).to(DEV)
    dzb = _normal(g, r64(T), N + 24)
    dzb[T:, OFF:OFF + N] = 0                                 # the zero tail of the operand; the rest of the buffer stays loud
    dw, wb = _window(N, 9 * Cin)
    yv.wgrad_conv3_gather(dzb.to(DEV)[:, OFF:OFF + N], yv.mview(xb, OFF, Cin), dw, B, Hin, Win, stride, tile_n=tile_n)
    return dw, wb


def run_case(yv, entry, tile_n, shape, split, slices) -> dict:
    """{"dw": hash of the dW window} of one case and "tail_kept": whether everything around the window kept its pre-fill"""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(entry, tile_n, shape, split, slices).encode()))
    with _split(yv, split):
        if entry in ("wgrad_tiled", "wgrad_wide"):
            dw, wb = _matrix(yv, g, entry, tile_n, shape, slices)
        elif entry == "wgrad_conv3_tiled":
            dw, wb = _conv3(yv, g, tile_n, shape, slices)
        else:
            dw, wb = _gather(yv, g, tile_n, shape, slices)
        torch.cuda.synchronize()
    res = {"dw": _sha(dw)}
    dw.fill_(SENT)
    res["tail_kept"] = bool((wb == SENT).all())
    return res


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
